"""T-CSR trim without a GPU: tg_tcsr_trim_host against the numpy reference (any trim) and against tg_tcsr_build_host over the
filtered events (a horizon alone) - all four arrays, bit for bit - and Graph.trimmed on host-only parents: what it
refuses, what it carries over, and that it composes with Graph.extended."""
import numpy as np
import pytest

from _append_ref import assert_same, host_append, host_build, stream
from _trim_ref import STREAMS, events, host_trim, max_degree, repeated_time, trim_by_build, trim_numpy, trims_of

TRIMS = [(name, *t) for name in STREAMS for t in trims_of(name)]


@pytest.mark.parametrize('name,label,t_cut,keep_last', TRIMS, ids=[f'{t[0]}-{t[1]}' for t in TRIMS])
def test_host_trim_equals_the_references(name, label, t_cut, keep_last):
    N, s = STREAMS[name]
    ev = events(s)
    h = host_build(N, *ev)
    before = [a.copy() for a in h]
    rc, got, kept = host_trim(h, t_cut, -1 if keep_last is None else keep_last)
    assert rc == 0
    assert_same(got, trim_numpy(h, t_cut, keep_last), f'{name} {label}')
    assert kept == got[0][-1] == len(got[1])
    if keep_last is None:
        assert_same(got, trim_by_build(N, ev, t_cut), f'{name} {label} (build over the filtered events)')
    assert_same(h, before, 'the input is only read')
    if label in ('copy', 'below-all', 'at-first', 'keep-maxdeg', 'keep-huge'):
        assert_same(got, h, 'identity')
    if label in ('above-all', '+inf', 'keep0'):
        assert kept == 0 and not got[0].any()
    if label == 'at-last':
        assert 0 < kept <= len(h[1])   # entries AT the cut stay


def test_entries_at_a_repeated_cut_time_stay_and_earlier_ones_go():
    N, s = STREAMS['N1000-E2048']
    ev = events(s)
    t = repeated_time(ev)
    assert (ev[2] == t).sum() > 2
    _, got, kept = host_trim(host_build(N, *ev), t)
    assert kept == 2 * int((ev[2] >= t).sum())
    assert got[1].min() == t and int((got[1] == t).sum()) == 2 * int((ev[2] == t).sum())


def test_horizon_and_cap_each_bind_on_some_node():
    N, s = STREAMS['N65-E201']
    ev = events(s)
    h = host_build(N, *ev)
    t, M = float(np.median(ev[2])), 3
    both, hor, cap = (np.diff(trim_numpy(h, a, b)[0]) for a, b in ((t, M), (t, None), (-np.inf, M)))
    assert (both < hor).any(), 'the cap binds nowhere'
    assert (both < cap).any(), 'the horizon binds nowhere'
    rc, got, _ = host_trim(h, t, M)
    assert rc == 0
    assert_same(got, trim_numpy(h, t, M), 'both')
    np.testing.assert_array_equal(np.diff(got[0]), np.minimum(hor, cap))


def test_a_self_loop_straddling_the_cap_keeps_only_its_flag_1_entry():
    N, s = STREAMS['self-loop']
    h = host_build(N, *events(s))
    assert h[2][h[0][4]:h[0][5]].tolist() == [1, 2, 3, 4, 4]
    _, (indptr, ts, nbr, eid), _ = host_trim(h, keep_last=1)
    row = slice(indptr[4], indptr[5])
    assert nbr[row].tolist() == [4] and ts[row].tolist() == [5.0]
    assert (eid[row].view(np.uint32) >> 31).tolist() == [1] and (eid[row].view(np.uint32) & 0x7FFFFFFF).tolist() == [13]
    _, (indptr, _, nbr, eid), _ = host_trim(h, keep_last=2)
    assert (eid[indptr[4]:indptr[5]].view(np.uint32) >> 31).tolist() == [0, 1]


def test_the_unsorted_stream_is_trimmed_in_its_per_node_time_order():
    N, s = STREAMS['unsorted']
    ev = events(s)
    assert not np.all(ev[2][1:] >= ev[2][:-1])
    h = host_build(N, *ev)
    for v in range(N):
        assert np.all(np.diff(h[1][h[0][v]:h[0][v + 1]]) >= 0)
    t = float(np.median(ev[2]))
    assert_same(host_trim(h, t)[1], trim_by_build(N, ev, t), 'unsorted')


def test_host_twin_refuses_nan_and_bad_graphs():
    import ctypes as C
    from www2023tiger_amd._lib import TG_EINVAL, TgTcsr, lib, ptr
    N, s = STREAMS['tiny']
    h = host_build(N, *events(s))
    assert host_trim(h, np.nan)[0] == TG_EINVAL
    out = (np.empty(N + 1, dtype=np.int64), np.empty(6, dtype=np.float64), np.empty(6, dtype=np.int32),
           np.empty(6, dtype=np.int32))
    kept = C.c_int64(0)
    for nn, ne in ((0, 6), (-1, 6), (2 ** 31, 6), (N, -1), (N, 2 ** 32)):
        g = TgTcsr(nn, ne, *(ptr(a) for a in h))
        assert lib.tg_tcsr_trim_host(C.byref(g), 0.0, -1, *(ptr(a) for a in out), C.byref(kept)) == TG_EINVAL
    assert lib.tg_tcsr_trim_workspace_bytes(0) == 0 and lib.tg_tcsr_trim_workspace_bytes(N) > 0


# -------------------------------------------------------------------------------------------- Graph.trimmed, host only
def graph_of(N, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(*ev, max_node_id=N - 1, **kw)


def test_trimmed_refuses_before_anything_changes():
    N, s = STREAMS['N65-E201']
    g = graph_of(N, events(s))
    with pytest.raises(ValueError, match='NaN'):
        g.trimmed(before=float('nan'))
    with pytest.raises(ValueError, match='NaN'):
        g.trimmed(before=np.float32('nan'), keep_last=3)
    with pytest.raises(ValueError, match='negative'):
        g.trimmed(keep_last=-1)
    with pytest.raises(TypeError):
        g.trimmed(keep_last=2.5)


@pytest.mark.parametrize('before,keep_last', [(None, None), (30.0, None), (None, 4), (30.0, 2), (1e9, None), (None, 0)])
def test_trimmed_on_a_host_only_parent(before, keep_last):
    N, s = STREAMS['N65-E201']
    ev = events(s)
    g0 = graph_of(N, ev, strategy='recent_edges', seed=3)
    g0.alpha = 0.25
    h0 = [a.copy() for a in g0._host_tcsr()]
    g1 = g0.trimmed(before=before, keep_last=keep_last)
    assert g1 is not g0 and g1.num_node == N and g1.serial != g0.serial
    want = trim_numpy(h0, -np.inf if before is None else before, keep_last)
    assert_same(g1._host_tcsr(), want, 'trimmed')
    assert_same(g0._host_tcsr(), h0, 'the parent is unchanged')
    assert len(g0._events[0]) == len(ev[0])
    assert (g1.strategy, g1.seed, g1.alpha, g1._device) == (g0.strategy, g0.seed, g0.alpha, g0._device)
    assert g1.rng is g0.rng and g1._time_ordered == g0._time_ordered
    assert g1._t_last == g0._t_last == ev[2].max()   # kept even when nothing else is
    assert not any(v is g0 for v in vars(g1).values()) and g1._root is not g0._root
    if keep_last is None:   # still the T-CSR of an event list
        m = ev[2] >= (-np.inf if before is None else before)
        for a, b in zip(g1._events, ev):
            np.testing.assert_array_equal(a, b[m])
    else:
        assert g1._events is None
    with pytest.raises(ValueError, match='before the latest event'):   # it still refuses to go back in time
        g1.extended(ev[0][:1], ev[1][:1], ev[2][-1:] - 1, ev[3][:1])


def test_extended_after_trimmed_after_extended_equals_the_reference_in_the_same_order():
    N, E = 90, 700
    s = events(stream(N, E, seed=31))
    part = lambda lo, hi: tuple(np.ascontiguousarray(a[lo:hi]) for a in s)
    t_cut = float(s[2][250])
    for before, keep_last in ((t_cut, None), (None, 5), (t_cut, 3)):
        g = graph_of(N, part(0, 200)).extended(*part(200, 400)).trimmed(before=before, keep_last=keep_last)
        g = g.extended(*part(400, 600)).extended(*part(600, E))
        h = host_append(N, host_build(N, *part(0, 200)), part(200, 400))[1]
        h = trim_numpy(h, -np.inf if before is None else before, keep_last)
        h = host_append(N, h, part(400, 600))[1]
        h = host_append(N, h, part(600, E))[1]
        assert_same(g._host_tcsr(), h, f'before={before} keep_last={keep_last}')
        if keep_last is None:
            assert_same(g._host_tcsr(), trim_by_build(N, s, t_cut), 'horizon alone: the build over the filtered stream')
            assert len(g._events[0]) == int((s[2] >= t_cut).sum())
        # a second trim on top
        g2 = g.trimmed(keep_last=2)
        assert_same(g2._host_tcsr(), trim_numpy(h, -np.inf, 2), 'trimmed twice')
        assert max_degree(g2._host_tcsr()) <= 2


def test_trimmed_on_an_unsorted_parent():
    N, s = STREAMS['unsorted']
    ev = events(s)
    g = graph_of(N, ev)
    assert not g._time_ordered
    t = float(np.median(ev[2]))
    assert_same(g.trimmed(before=t)._host_tcsr(), trim_by_build(N, ev, t), 'unsorted parent')
    assert_same(g.trimmed(before=t, keep_last=2)._host_tcsr(), trim_numpy(host_build(N, *ev), t, 2), 'unsorted parent, cap')
