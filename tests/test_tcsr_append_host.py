"""T-CSR extension without a GPU: tg_tcsr_append_host against tg_tcsr_build_host over [old events | new events] - all four
arrays, bit for bit - and Graph.extended on a host-only parent: the lazily produced host view, what it refuses, what it
carries over."""
import numpy as np
import pytest
import torch

from _append_ref import CASES, assert_same, cut, host_append, host_build, reference, stream


@pytest.mark.parametrize('case', list(CASES))
def test_host_append_equals_host_build_over_the_concatenation(case):
    N, old, new = cut(case)
    rc, got = host_append(N, host_build(N, *old), new)
    assert rc == 0
    assert_same(got, reference(N, old, new), case)
    if case == 'n0':
        assert len(new[0]) == 0
        assert_same(got, host_build(N, *old), 'n = 0 copies')


def test_rows_are_old_rows_followed_by_new_entries_and_a_self_loop_keeps_flag_order():
    N, old, new = cut('tiny-1+2')
    h0 = host_build(N, *old)
    _, (indptr, ts, nbr, eid) = host_append(N, h0, new)
    # node 3: the old self loop (flag 0 then flag 1), then event 2 seen from its source, then event 3 seen from its destination
    row = slice(indptr[3], indptr[4])
    assert nbr[row].tolist() == [3, 3, 2, 1]
    assert (eid[row].view(np.uint32) & 0x7FFFFFFF).tolist() == [1, 1, 2, 3]
    assert (eid[row].view(np.uint32) >> 31).tolist() == [0, 1, 0, 1]
    assert ts[row].tolist() == [1.0, 1.0, 1.0, 2.0]
    for v in range(N):   # every row starts with the node's old row
        lo, n_old = h0[0][v], h0[0][v + 1] - h0[0][v]
        assert nbr[indptr[v]:indptr[v] + n_old].tolist() == h0[2][lo:lo + n_old].tolist()


def test_a_chain_of_five_appends_equals_one_build():
    N, E = 120, 1500
    s = stream(N, E, seed=21)
    cuts = [200, 201, 640, 640, 1100, E]   # a single event and an empty batch among them
    h = host_build(N, *(a[:cuts[0]] for a in s))
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        rc, h = host_append(N, h, tuple(np.ascontiguousarray(a[lo:hi]) for a in s))
        assert rc == 0
    assert_same(h, host_build(N, *s), 'chain')


def test_host_twin_refuses_bad_ids_and_eids():
    N, old, new = cut('N65-E1-n200')
    h = host_build(N, *old)
    for col, val in ((0, N), (0, -1), (1, N), (3, 2 ** 31), (3, -1)):
        bad = [a.copy() for a in new]
        bad[col][17] = val
        assert host_append(N, h, tuple(bad))[0] == -1   # TG_EINVAL


# ------------------------------------------------------------------------------------------- Graph.extended, host only
def graph_of(N, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(*ev, max_node_id=N - 1, **kw)


@pytest.mark.parametrize('case', ['tiny-1+2', 'N1000-E1023-n1025', 'first-ts-equal-t-last', 'n0'])
def test_extended_on_a_host_only_parent(case):
    N, old, new = cut(case)
    g0 = graph_of(N, old, strategy='recent_nodes', seed=3)
    before = [a.copy() for a in g0._host_tcsr()]
    g1 = g0.extended(*new)
    assert g1 is not g0 and g1.num_node == N and g1.serial != g0.serial
    assert_same(g1._host_tcsr(), reference(N, old, new), case)
    for a, b in zip(g1._events, (np.concatenate([x, y]) for x, y in zip(old, new))):
        np.testing.assert_array_equal(a, b)
    assert_same(g0._host_tcsr(), before, 'the parent is unchanged')
    assert len(g0._events[0]) == len(old[0])
    assert (g1.strategy, g1.seed, g1.alpha, g1._device) == (g0.strategy, g0.seed, g0.alpha, g0._device)
    assert g1.rng is g0.rng   # one random stream


def test_extended_takes_cpu_tensors_and_chains():
    N, E = 90, 700
    s = stream(N, E, seed=31)
    g = graph_of(N, tuple(a[:100] for a in s))
    for lo, hi in ((100, 101), (101, 400), (400, 400), (400, E)):
        g = g.extended(*(torch.from_numpy(a[lo:hi]) for a in s))
    assert_same(g._host_tcsr(), host_build(N, *s), 'chain of extended')
    assert len(g._events[0]) == E


def test_extended_on_parents_of_the_host_builder():
    """an adjacency-list parent and an unsorted stream: both are built by the host routine and both are extendable"""
    from www2023tiger_amd.data.graph import Graph
    N, old, new = cut('N65-E1-n200')
    N2, E0 = 50, 300
    s = stream(N2, 400, seed=41)
    perm = np.random.RandomState(0).permutation(E0)
    old2 = tuple(np.ascontiguousarray(a[:E0][perm]) for a in s)
    new2 = tuple(np.ascontiguousarray(a[E0:]) for a in s)
    g = graph_of(N2, old2)
    assert not g._time_ordered
    want = host_build(N2, *(np.concatenate([a, b]) for a, b in zip(old2, new2)))
    assert_same(g.extended(*new2)._host_tcsr(), want, 'unsorted parent')
    adj = [[] for _ in range(N)]
    for s_, d_, t_, e_ in zip(*old):
        adj[s_].append((d_, e_, t_, 0))
        adj[d_].append((s_, e_, t_, 1))
    ga = Graph(adj, strategy='recent_edges', seed=0)
    assert_same(ga.extended(*new)._host_tcsr(), reference(N, old, new), 'adjacency-list parent')


def test_extended_refuses_before_anything_changes():
    N, old, new = cut('N65-E1-n200')
    s = stream(N, 300, seed=51)
    g = graph_of(N, tuple(a[:150] for a in s))
    new = tuple(a[150:].copy() for a in s)

    def bad(col, idx, val):
        b = [a.copy() for a in new]
        b[col][idx] = val
        return b
    with pytest.raises(ValueError, match='non-decreasing'):
        g.extended(*bad(2, 40, new[2][39] - 1))
    with pytest.raises(ValueError, match='non-decreasing'):
        g.extended(*bad(2, 40, np.nan))
    with pytest.raises(ValueError, match='before the latest event'):
        g.extended(*bad(2, 0, s[2][149] - 1))
    for col, val in ((0, N), (1, -1)):
        with pytest.raises(ValueError, match='node ids'):
            g.extended(*bad(col, 3, val))
    for val in (2 ** 31, -1):
        with pytest.raises(ValueError, match='31 bits'):
            g.extended(*bad(3, 3, val))
    with pytest.raises(ValueError, match='one entry per event'):
        g.extended(new[0], new[1][:-1], new[2], new[3])
    # an extended graph keeps its own t_last: what its parent would take, it refuses
    g1 = g.extended(*new)
    with pytest.raises(ValueError, match='before the latest event'):
        g1.extended(*new)
    assert len(g._events[0]) == 150 and len(g1._events[0]) == 300


def test_serials_are_unique_and_the_adversarial_sampler_follows_its_graph():
    """the sampler's pair index is sized by the graph it was built for: with an extended graph in its place it rebuilds
    (and then finds that the graph is no longer the one over its full stream) instead of indexing past the stale arrays"""
    from www2023tiger_amd.data.adversarial import AdversarialEdgeSampler
    N, E = 60, 500
    s = stream(N, E + 40, seed=61)
    src, dst, ts = (a[:E] for a in s[:3])
    g = graph_of(N, (src, dst, ts, np.arange(E, dtype=np.int64)))
    smp = AdversarialEdgeSampler(src, dst, ts, src[-100:], ts[-100:], 'hist', seed=1, graph=g, device='cpu')
    first = smp.sample(src[-100:], ts[-100], ts[-1])[1]
    assert smp._ix_serial == g.serial
    g2 = g.extended(*(a[E:] for a in s[:3]), np.arange(E, E + 40, dtype=np.int64))
    assert len({g.serial, g2.serial, graph_of(N, (src, dst, ts, s[3][:E])).serial}) == 3
    smp.graph = g2
    with pytest.raises(ValueError, match='not over the full stream'):
        smp.sample(src[-100:], ts[-100], ts[-1])
    smp.graph = g   # back on its own graph: rebuilt once more, the same draws as a fresh sampler
    smp.reset_random_state()
    np.testing.assert_array_equal(smp.sample(src[-100:], ts[-100], ts[-1])[1], first)
