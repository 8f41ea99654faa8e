"""Late events without a GPU: tg_tcsr_merge_host against a numpy reference (stable per-row sort of [old row | new entries]) and
against tg_tcsr_build_host over [old events | batch] - all four arrays, bit for bit - and Graph.merged on a host-only
parent: the event list it keeps, the time-ordered flag, what it refuses, what it carries over."""
import numpy as np
import pytest
import torch

from _append_ref import host_append
from _merge_ref import CASES, as_batch, assert_same, concat, host_build, host_merge, late_batch, np_merge, stream


def test_symbols_resolve_and_the_abi_version_stays_9():
    from www2023tiger_amd import _lib
    for name in ('tg_tcsr_merge_workspace_bytes', 'tg_tcsr_merge', 'tg_tcsr_merge_host'):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert _lib.lib.tg_abi_version() == 9
    # the workspace convention of tg_tcsr_append_grow: 0 for nothing to sort and for arguments the call refuses
    ws = _lib.lib.tg_tcsr_merge_workspace_bytes
    assert ws(100, 0, 5, 5) == 0 and ws(100, 3, 5, 4) == 0 and ws(-1, 3, 5, 5) == 0 and ws(100, 3, 5, 5) > 0


@pytest.mark.parametrize('case', list(CASES))
def test_host_merge_equals_numpy_and_the_host_build_over_the_concatenation(case):
    from www2023tiger_amd.hip_ops import tcsr_verify_host
    N0, N, old, new = CASES[case]
    h = host_build(N0, *old)
    rc, got = host_merge(h, N, new)
    assert rc == 0
    assert_same(got, np_merge(h, N, new), case + ' (numpy)')
    assert_same(got, host_build(N, *concat(old, new)), case + ' (host build)')
    assert tcsr_verify_host(got)[0] == 0
    if case in ('n0', 'growth-n0'):
        assert len(new[0]) == 0
        for a, b in zip(got[1:], h[1:]):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg='n = 0 copies')
    if case == 'all-after-ordered':
        rc, want = host_append(N, h, new)
        assert rc == 0
        assert_same(got, want, 'a batch the append takes gives the append\'s bytes')


def test_equal_times_keep_old_entries_first_and_new_ones_in_entry_order():
    N0, N, old, new = CASES['all-equal']
    h = host_build(N0, *old)
    _, (indptr, ts, nbr, eid) = host_merge(h, N, new)
    j = np.arange(2 * len(new[0]))
    owner = np.where(j & 1, new[1][j >> 1], new[0][j >> 1])
    for v in range(N):
        n_old = h[0][v + 1] - h[0][v]
        row = slice(indptr[v], indptr[v + 1])
        np.testing.assert_array_equal(eid[row][:n_old], h[3][h[0][v]:h[0][v + 1]])   # the old row, in place
        mine = j[owner == v]
        want = new[3][mine >> 1].astype(np.uint32) | ((mine & 1).astype(np.uint32) << np.uint32(31))
        np.testing.assert_array_equal(eid[row][n_old:].view(np.uint32), want)         # then the new ones by ascending j


def test_signed_zeros_order_by_equality_and_keep_their_bits():
    """old row of node 1: [-0.0, +0.0]; late entries at +0.0, -0.0, -1.0, +0.0: the -1.0 goes first, the three zeros go
    BEHIND both old zeros in batch order, every sign bit as it came (a key built from the raw bits would put -0.0 first)"""
    old = as_batch(([1, 1], [2, 2], [-0.0, 0.0], [10, 11]))
    new = as_batch(([1, 1, 1, 1], [3, 3, 3, 3], [0.0, -0.0, -1.0, 0.0], [20, 21, 22, 23]))
    h = host_build(4, *old)
    rc, (indptr, ts, nbr, eid) = host_merge(h, 4, new)
    assert rc == 0
    row = slice(indptr[1], indptr[2])
    assert eid[row].tolist() == [22, 10, 11, 20, 21, 23]
    assert np.signbit(ts[row]).tolist() == [True, True, False, False, True, False]
    assert_same((indptr, ts, nbr, eid), host_build(4, *concat(old, new)), 'zeros')


def test_a_self_loop_keeps_flag_order_and_infinities_sort_to_the_ends():
    old = as_batch(([2], [2], [1.0], [5]))
    new = as_batch(([2, 2, 2], [2, 1, 2], [np.inf, -np.inf, 1.0], [6, 7, 8]))
    rc, (indptr, ts, nbr, eid) = host_merge(host_build(3, *old), 3, new)
    assert rc == 0
    row = slice(indptr[2], indptr[3])
    assert ts[row].tolist() == [-np.inf, 1.0, 1.0, 1.0, 1.0, np.inf, np.inf]
    assert (eid[row].view(np.uint32) & 0x7FFFFFFF).tolist() == [7, 5, 5, 8, 8, 6, 6]
    assert (eid[row].view(np.uint32) >> 31).tolist() == [0, 0, 1, 0, 1, 0, 1]


def test_host_twin_refuses_bad_ids_eids_and_nan():
    N0, N, old, new = CASES['growth']
    h = host_build(N0, *old)
    for col, val in ((0, N), (0, -1), (1, N), (3, 2 ** 31), (3, -1), (2, np.nan)):
        bad = [a.copy() for a in new]
        bad[col][17] = val
        assert host_merge(h, N, tuple(bad))[0] == -1   # TG_EINVAL
    assert host_merge(h, N0 - 1, new)[0] == -1        # num_node_out below num_node


# --------------------------------------------------------------------------------------------- Graph.merged, host only
def graph_of(N, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(*ev, max_node_id=N - 1, **kw)


@pytest.mark.parametrize('case', ['empty-old', 'n0', 'all-before', 'all-after-ordered', 'inside', 'signed-zeros', 'hub', 'growth'])
def test_merged_on_a_host_only_parent(case):
    from www2023tiger_amd.hip_ops import tcsr_verify_host
    N0, N, old, new = CASES[case]
    g0 = graph_of(N0, old, strategy='recent_nodes', seed=3)
    before = [a.copy() for a in g0._host_tcsr()]
    g1 = g0.merged(*new, num_node=None if N == N0 else N)
    assert g1 is not g0 and g1.num_node == N and g1.serial != g0.serial and g1._log is None and g1._root is not g0._root
    want = host_build(N, *concat(old, new))
    assert_same(g1._host_tcsr(), want, case)
    assert tcsr_verify_host(g1)[0] == 0
    assert_same(g0._host_tcsr(), before, 'the parent is unchanged')
    assert len(g0._events[0]) == len(old[0]) and g0.num_node == N0
    # the event list is the concatenation, and a graph rebuilt from it - by whichever builder the flag selects - is the same
    for a, b in zip(g1._events, concat(old, new)):
        np.testing.assert_array_equal(a, b)
    full = concat(old, new)[2]
    assert g1._time_ordered == bool(np.all(full[1:] >= full[:-1]))
    rebuilt = graph_of(N, g1._events)
    assert rebuilt._time_ordered == g1._time_ordered
    assert_same(rebuilt._host_tcsr(), want, case + ' (rebuilt from _events)')
    t_all = np.concatenate([old[2], new[2]])
    assert g1._t_last == (t_all.max() if len(t_all) else -np.inf)
    assert (g1.strategy, g1.seed, g1.alpha, g1._device) == (g0.strategy, g0.seed, g0.alpha, g0._device)
    assert g1.rng is g0.rng   # one random stream


def test_merged_auto_num_node_and_cpu_tensors():
    N0, N, old, new = CASES['growth-new-ids-only']
    g = graph_of(N0, old).merged(*(torch.from_numpy(a) for a in new), num_node='auto')
    n_auto = int(max(new[0].max(), new[1].max())) + 1
    assert g.num_node == n_auto
    assert_same(g._host_tcsr(), host_build(n_auto, *concat(old, new)), 'auto')


def test_merged_refuses_before_anything_changes_and_does_not_refuse_disorder():
    N0, N, old, new = CASES['inside']
    g = graph_of(N0, old)
    before = [a.copy() for a in g._host_tcsr()]

    def bad(col, idx, val):
        b = [a.copy() for a in new]
        b[col][idx] = val
        return b
    with pytest.raises(ValueError, match='NaN'):
        g.merged(*bad(2, 40, np.nan))
    for col, val in ((0, N0), (1, -1)):
        with pytest.raises(ValueError, match='node ids'):
            g.merged(*bad(col, 3, val))
    with pytest.raises(ValueError, match='node ids'):
        g.merged(*bad(0, 3, N0 + 5), num_node=N0 + 5)
    for val in (2 ** 31, -1):
        with pytest.raises(ValueError, match='31 bits'):
            g.merged(*bad(3, 3, val))
    with pytest.raises(ValueError, match='no row of the edge table'):
        g.merged(*bad(3, 3, 1000), eid_rows=1000)
    with pytest.raises(ValueError, match='one entry per event'):
        g.merged(new[0], new[1][:-1], new[2], new[3])
    with pytest.raises(ValueError, match='below the graph'):
        g.merged(*new, num_node=N0 - 1)
    with pytest.raises(ValueError, match="'auto'"):
        g.merged(*new, num_node='grow')
    assert_same(g._host_tcsr(), before, 'nothing changed')
    # the same batch goes back in time: `extended` refuses it as ever, `merged` takes it
    with pytest.raises(ValueError, match='non-decreasing|before the latest event'):
        g.extended(*new)
    assert g.merged(*new)._host_tcsr()[1].shape == (2 * (len(old[0]) + len(new[0])),)


def test_a_chain_merged_extended_trimmed_merged_against_numpy():
    from www2023tiger_amd.hip_ops import tcsr_verify_host
    N = 80
    s = stream(N, 900, seed=23)
    old = as_batch(tuple(a[:500] for a in s))
    t_hi = float(s[2][499])
    b1 = late_batch(N, 140, 24, -3, t_hi)
    b2 = as_batch(tuple(a[500:700] for a in s))
    b3 = late_batch(N + 9, 160, 25, t_hi / 3, float(s[2][699]) + 5)
    g = graph_of(N, old)
    g1 = g.merged(*b1)
    g2 = g1.extended(*b2)
    g3 = g2.trimmed(before=t_hi / 3, keep_last=12)
    g4 = g3.merged(*b3, num_node=N + 9)
    assert g3._events is None and g4._events is None and not g4._time_ordered
    # the same chain in numpy: merge, append (a merge of an on-time batch), trim, merge
    h = np_merge(host_build(N, *old), N, b1)
    assert_same(g1._host_tcsr(), h, 'merged')
    h = np_merge(h, N, b2)
    assert_same(g2._host_tcsr(), h, 'merged -> extended')
    keep, kept = np.zeros(len(h[1]), dtype=bool), [0]
    for v in range(N):
        lo, hi = h[0][v], h[0][v + 1]
        first = max(lo + np.searchsorted(h[1][lo:hi], t_hi / 3, side='left'), hi - 12)
        keep[first:hi] = True
        kept.append(kept[-1] + hi - first)
    indptr = np.asarray(kept, dtype=np.int64)
    h = (indptr, h[1][keep], h[2][keep], h[3][keep])
    assert_same(g3._host_tcsr(), h, 'merged -> extended -> trimmed')
    assert_same(g4._host_tcsr(), np_merge(h, N + 9, b3), 'merged -> extended -> trimmed -> merged')
    for x in (g1, g2, g3, g4):
        assert tcsr_verify_host(x)[0] == 0
    assert g4._t_last == max(float(s[2][699]), float(b3[2].max()))
