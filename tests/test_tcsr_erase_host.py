"""T-CSR erase without a GPU: tg_tcsr_erase_host against the numpy reference and against tg_tcsr_build_host over the
filtered events - all four arrays, bit for bit - and Graph.without on host-only parents: what it refuses, what it carries
over, and that it composes with Graph.extended."""
import os
import subprocess

import numpy as np
import pytest

from _append_ref import assert_same, host_build, stream
from _erase_ref import bitmap, erase_by_build, erase_numpy, filtered, host_erase, keep_mask, small_eids
from _trim_ref import STREAMS, events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [n for n in STREAMS if n != 'unsorted']   # random, time-ordered: multi-edges, self loops, equal timestamps


def case(name):
    N, s = STREAMS[name]
    ev = small_eids(events(s))
    return N, ev, host_build(N, *ev)


def picks(N, ev, seed=0):
    """S: some nodes that occur (never 0), R: some eids of the stream, one of them a self loop's if there is one"""
    rs = np.random.RandomState(seed)
    ids = np.unique(np.concatenate([ev[0], ev[1]]))
    ids = ids[ids != 0]
    S = rs.choice(ids, size=max(1, len(ids) // 5), replace=False) if len(ids) else np.zeros(0, dtype=np.int64)
    R = rs.choice(ev[3], size=max(1, len(ev[3]) // 4), replace=False)
    loops = ev[3][ev[0] == ev[1]]
    if len(loops):
        R = np.concatenate([R, loops[:1]])
    return S.astype(np.int64), R.astype(np.int64)


@pytest.mark.parametrize('what', ['S', 'R', 'both'])
@pytest.mark.parametrize('name', NAMES)
def test_host_erase_equals_the_references(name, what):
    N, ev, h = case(name)
    S, R = picks(N, ev)
    S, R = (S if what != 'R' else None), (R if what != 'S' else None)
    before = [a.copy() for a in h]
    rc, got, kept = host_erase(h, S, R)
    assert rc == 0
    assert_same(got, erase_numpy(h, S, R), f'{name} {what}')
    assert_same(got, erase_by_build(N, ev, S, R), f'{name} {what} (build over the filtered events)')
    assert kept == got[0][-1] == len(got[1]) and kept % 2 == 0   # both entries of an event go together
    assert_same(h, before, 'the input is only read')
    if S is not None and len(S):
        assert not np.diff(got[0])[S].any(), 'an erased node owns an empty row'
        assert not np.isin(got[2], S).any()
    if name != 'N2-E1' or what == 'R':
        assert kept < len(h[1]), 'nothing was dropped: the case checks nothing'


def test_a_self_loop_loses_both_entries_together():
    N, ev, h = case('self-loop')
    assert h[2][h[0][4]:h[0][5]].tolist() == [1, 2, 3, 4, 4]
    loop_eid = int(ev[3][(ev[0] == 4) & (ev[1] == 4)][0])
    rc, got, kept = host_erase(h, None, [loop_eid])
    assert rc == 0 and kept == len(h[1]) - 2
    assert got[2][got[0][4]:got[0][5]].tolist() == [1, 2, 3]
    assert_same(got, erase_by_build(N, ev, None, [loop_eid]), 'self loop')


def test_a_marked_neighbour_goes_from_a_row_whose_owner_stays():
    N, ev, h = case('N65-E201')
    deg = np.diff(h[0])
    i = int(np.nonzero((ev[0] != ev[1]) & (deg[ev[0]] > 3))[0][0])
    v, u = int(ev[0][i]), int(ev[1][i])
    rc, got, _ = host_erase(h, [u], None)
    assert rc == 0
    old, new = h[2][h[0][v]:h[0][v + 1]], got[2][got[0][v]:got[0][v + 1]]
    assert 0 < len(new) < len(old) and u in old and u not in new
    assert new.tolist() == [x for x in old.tolist() if x != u]   # order kept


@pytest.mark.parametrize('name', ['tiny', 'N65-E201', 'hub'])
def test_nothing_marked_is_a_copy_and_everything_marked_is_empty(name):
    N, ev, h = case(name)
    for S, R in (([], None), (None, []), ([], []), (None, None), (None, [len(ev[0]) + 5])):   # the last: an absent eid
        rc, got, kept = host_erase(h, S, R)
        assert rc == 0 and kept == len(h[1])
        assert_same(got, h, f'copy S={S} R={R}')
    for S, R in ((np.arange(1, N), None), (None, ev[3]), (np.arange(1, N), ev[3])):
        rc, got, kept = host_erase(h, S, R)
        left = 0 if R is not None else 2 * int(((ev[0] == 0) & (ev[1] == 0)).sum())   # (node 0 talking to itself)
        assert rc == 0 and kept == left and got[0][-1] == left and len(got[0]) == N + 1
        assert not got[0][:-1].any() and got[0].dtype == np.int64


def test_duplicate_ids_and_an_n_rows_below_the_largest_eid():
    N, ev, h = case('N1000-E2048')
    S, R = picks(N, ev, seed=4)
    rc, got, _ = host_erase(h, np.concatenate([S, S, S[:3]]), np.concatenate([R, R]))
    assert rc == 0
    assert_same(got, erase_numpy(h, S, R), 'duplicates')
    n_rows = int(np.sort(R)[len(R) // 2])   # half of R lies at or beyond it: not retracted
    rc, got, kept = host_erase(h, None, R, n_rows=n_rows)
    assert rc == 0
    assert_same(got, erase_numpy(h, None, R, n_rows), 'n_rows')
    assert_same(got, erase_by_build(N, ev, None, R[R < n_rows]), 'n_rows (build)')
    assert kept > host_erase(h, None, R)[2]
    # the arbitrary 31-bit eids of the raw stream, bit 31 set on half of the entries: the bitmap covers 100 ids
    N, s = STREAMS['N65-E201']
    raw = events(s)
    hr = host_build(N, *raw)
    assert (hr[3] < 0).any() and int(raw[3].max()) == 0x7FFFFFFF
    rc, got, kept = host_erase(hr, None, np.arange(100), n_rows=100)
    assert rc == 0
    assert_same(got, erase_numpy(hr, None, np.arange(100), 100), 'raw eids')


def test_host_twin_refuses_bad_graphs_and_a_negative_n_rows():
    import ctypes as C
    from www2023tiger_amd._lib import TG_EINVAL, TgTcsr, lib, ptr
    N, ev, h = case('tiny')
    P = len(h[1])
    out = (np.full(N + 1, -7, dtype=np.int64), np.empty(P, dtype=np.float64), np.empty(P, dtype=np.int32),
           np.empty(P, dtype=np.int32))
    kept = C.c_int64(-1)
    nb = bitmap([3], N)
    for nn, ne in ((0, P), (-1, P), (2 ** 31, P), (N, -1), (N, 2 ** 32)):
        g = TgTcsr(nn, ne, *(ptr(a) for a in h))
        assert lib.tg_tcsr_erase_host(C.byref(g), ptr(nb), None, 0, *(ptr(a) for a in out), C.byref(kept)) == TG_EINVAL
    g = TgTcsr(N, P, *(ptr(a) for a in h))
    assert lib.tg_tcsr_erase_host(C.byref(g), ptr(nb), ptr(nb), -1, *(ptr(a) for a in out), C.byref(kept)) == TG_EINVAL
    assert kept.value == -1 and (out[0] == -7).all(), 'something was written'
    assert lib.tg_tcsr_erase_workspace_bytes(0, 10) == 0 and lib.tg_tcsr_erase_workspace_bytes(N, -1) == 0
    assert lib.tg_tcsr_erase_workspace_bytes(N, 2 ** 32) == 0
    # 256 bytes of keep bits per tile of 2048 entries, a count per tile, a base per tile and one more; 16-byte parts
    al = lambda x: (x + 15) // 16 * 16
    for ne in (0, 1, 2047, 2048, 2049, 4097, 10 ** 6):
        t = (ne + 2047) // 2048
        assert lib.tg_tcsr_erase_workspace_bytes(N, ne) == al(256 * t) + al(4 * t) + al(4 * (t + 1))


def test_the_new_symbols_resolve_and_the_abi_version_stands():
    from www2023tiger_amd import _lib
    assert _lib.lib.tg_abi_version() == 9
    for name in ('tg_tcsr_erase_workspace_bytes', 'tg_tcsr_erase_plan', 'tg_tcsr_erase_apply', 'tg_tcsr_erase_host'):
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None
    text = open(os.path.join(ROOT, 'include', 'tiger_hip.h')).read()
    assert '#define TG_ABI_VERSION 9' in text
    for name in ('tg_tcsr_erase_workspace_bytes(', 'tg_tcsr_erase_plan(', 'tg_tcsr_erase_apply(', 'tg_tcsr_erase_host('):
        assert name in text


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / 'abi.c'
    src.write_text('#include "tiger_hip.h"\n'
                   'size_t (*a)(int64_t, int64_t) = tg_tcsr_erase_workspace_bytes;\n'
                   'int (*b)(const tg_tcsr*, const int64_t*, const int64_t*, int64_t, int64_t*, void*, size_t, void*) = '
                   'tg_tcsr_erase_plan;\n'
                   'int (*c)(const tg_tcsr*, const int64_t*, int64_t, double*, int32_t*, int32_t*, const void*, size_t, void*) = '
                   'tg_tcsr_erase_apply;\n'
                   'int (*d)(const tg_tcsr*, const int64_t*, const int64_t*, int64_t, int64_t*, double*, int32_t*, int32_t*, '
                   'int64_t*) = tg_tcsr_erase_host;\n'
                   'int main(void) { return TG_ABI_VERSION == 9 ? 0 : 1; }\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', os.path.join(ROOT, 'include'), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# -------------------------------------------------------------------------------------------- Graph.without, host only
def graph_of(N, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(*ev, max_node_id=N - 1, **kw)


def test_without_refuses_before_anything_changes():
    import torch
    N, ev, _ = case('N65-E201')
    g = graph_of(N, ev)
    serial = g.serial
    with pytest.raises(ValueError, match='padding id'):
        g.without(nodes=[3, 0])
    with pytest.raises(ValueError, match='padding id'):
        g.without(nodes=torch.tensor([0]))
    with pytest.raises(ValueError, match=r'\[0, num_node\)'):
        g.without(nodes=[N])
    with pytest.raises(ValueError, match=r'\[0, num_node\)'):
        g.without(nodes=[-1], eids=[3])
    with pytest.raises(ValueError, match='non-negative'):
        g.without(eids=[4, -1])
    with pytest.raises(ValueError, match='non-negative'):
        g.without(eids=[2 ** 31])
    with pytest.raises(ValueError, match='both None'):
        g.without()
    with pytest.raises(ValueError, match='integer ids'):
        g.without(nodes=[1.5])
    with pytest.raises(ValueError, match='eid_rows'):
        g.without(eids=[1], eid_rows=-1)
    assert g.serial == serial and len(g._events[0]) == len(ev[0])


@pytest.mark.parametrize('what', ['S', 'R', 'both', 'all', 'none', 'absent'])
def test_without_on_a_host_only_parent(what):
    import torch
    N, ev, h = case('N65-E201')
    S, R = picks(N, ev, seed=2)
    S, R = {'S': (S, None), 'R': (None, R), 'both': (S, R), 'all': (np.arange(1, N), ev[3]), 'none': ([], []),
            'absent': (None, [10 ** 6])}[what]
    g0 = graph_of(N, ev, strategy='recent_edges', seed=3)
    g0.alpha = 0.25
    h0 = [a.copy() for a in g0._host_tcsr()]
    # (tensors and duplicates are as good as lists)
    g1 = g0.without(nodes=None if S is None else torch.as_tensor(np.concatenate([S, S]).astype(np.int64)), eids=None if R is None else list(R))
    assert g1 is not g0 and g1.num_node == N and g1.serial != g0.serial and g1._dev is None
    want = erase_numpy(h0, S, R)
    assert_same(g1._host_tcsr(), want, what)
    assert_same(g1._host_tcsr(), erase_by_build(N, ev, S, R), f'{what} (build)')
    assert_same(g0._host_tcsr(), h0, 'the parent is unchanged')
    assert len(g0._events[0]) == len(ev[0])
    assert (g1.strategy, g1.seed, g1.alpha, g1._device) == (g0.strategy, g0.seed, g0.alpha, g0._device)
    assert g1.rng is g0.rng and g1._time_ordered == g0._time_ordered
    assert g1._t_last == g0._t_last == ev[2].max()   # kept even when nothing else is
    assert not any(v is g0 for v in vars(g1).values()) and g1._root is not g0._root
    for a, b in zip(g1._events, filtered(ev, S, R)):   # still the T-CSR of an event list
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a, b)
    if what in ('none', 'absent'):
        assert_same(g1._host_tcsr(), h0, 'a copy')
    if what == 'all':
        assert len(g1._host_tcsr()[1]) == 0
    with pytest.raises(ValueError, match='before the latest event'):   # it still refuses to go back in time
        g1.extended(ev[0][:1], ev[1][:1], ev[2][-1:] - 1, ev[3][:1])
    # `extended` still works on it - an erased id comes back as a node never seen
    back = int(np.asarray(S)[0]) if S is not None and len(S) else 5
    new = (np.array([back, 7]), np.array([9, back]), ev[2][-1:].repeat(2) + 1.0, np.array([3000, 3001]))
    g2 = g1.extended(*new)
    full = tuple(np.concatenate([a, np.asarray(b, dtype=a.dtype)]) for a, b in zip(filtered(ev, S, R), new))
    assert_same(g2._host_tcsr(), host_build(N, *full), f'{what}: extended after without')


def test_eid_rows_bounds_what_is_retracted():
    N, ev, h = case('N65-E201')
    g = graph_of(N, ev)
    R = np.array([5, 50, 150])
    assert_same(g.without(eids=R, eid_rows=100)._host_tcsr(), erase_by_build(N, ev, None, [5, 50]), 'eid_rows')
    assert len(g.without(eids=R, eid_rows=100)._events[0]) == len(ev[0]) - 2
    assert_same(g.without(eids=R, eid_rows=0)._host_tcsr(), h, 'eid_rows = 0')


def test_without_after_extended_and_on_a_parent_without_an_event_list():
    N, E = 90, 700
    s = small_eids(events(stream(N, E, seed=31)))
    part = lambda lo, hi: tuple(np.ascontiguousarray(a[lo:hi]) for a in s)
    S, R = picks(N, s, seed=7)
    g = graph_of(N, part(0, 300)).extended(*part(300, E))
    assert_same(g.without(S, R)._host_tcsr(), erase_by_build(N, s, S, R), 'without after extended')
    t = g.trimmed(keep_last=4)   # no event list any more
    assert t._events is None
    w = t.without(S, R)
    assert w._events is None
    assert_same(w._host_tcsr(), erase_numpy(t._host_tcsr(), S, R), 'without after a cap')


def test_memory_clear_of_some_ids_zeroes_their_rows_and_nothing_else():
    import torch
    from www2023tiger_amd.model.memory import Memory
    m = Memory(70, 4)
    m.vals.copy_(torch.arange(280, dtype=torch.float32).reshape(70, 4) + 1)
    m.update_ts.copy_(torch.arange(70, dtype=torch.float32) + 1)
    m.active_mask.fill_(True)
    before = (m.vals.clone(), m.update_ts.clone(), m.active_mask.clone())
    v0 = m._version_
    ids = torch.tensor([3, 64, 69, 3])
    m.clear(ids)
    assert m._version_ > v0
    others = torch.ones(70, dtype=torch.bool)
    others[ids] = False
    for now, was in zip((m.vals, m.update_ts, m.active_mask), before):
        assert not bool(now[ids].any()) and torch.equal(now[others], was[others])
    m.clear(torch.zeros(0, dtype=torch.int64))
    assert torch.equal(m.vals[others], before[0][others])
    for bad in ([70], [-1]):
        with pytest.raises(ValueError, match='outside'):
            m.clear(torch.tensor(bad))
    assert torch.equal(m.vals[others], before[0][others])
    m.clear()   # the whole-table form is what it was
    assert not bool(m.vals.any()) and not bool(m.update_ts.any()) and not bool(m.active_mask.any())
