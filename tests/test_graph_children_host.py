"""What every graph derived from a graph carries over, without a GPU: Graph.extended, widened, trimmed, without and
renumbered on one host-only parent (65 nodes, 201 events).  The child keeps strategy, seed, alpha, the parent's `rng` object,
the time-ordered flag and the latest event time (advanced by an extension), has a serial of its own and leaves the parent's
host arrays as they were.  The device MT19937 state follows one rule: the child of `extended` (and of `widened`, which is an
extension by no events) starts without one and re-derives it from the shared `rng` on first use; every other child holds its
parent's."""
import numpy as np
import pytest

from _append_ref import stream

N, EV = 65, tuple(np.ascontiguousarray(a) for a in stream(65, 201, seed=2))
T_LAST = float(EV[2].max())
NEW = (np.array([3, 64]), np.array([9, 3]), np.array([T_LAST, T_LAST + 2.0]), np.array([7, 8]))

# name -> (the derivation, the child's num_node, the child's latest event time)
CHILDREN = {
    'extended': (lambda g: g.extended(*NEW), N, T_LAST + 2.0),
    'extended-grown': (lambda g: g.extended(*NEW, num_node=N + 5), N + 5, T_LAST + 2.0),
    'widened': (lambda g: g.widened(N + 5), N + 5, T_LAST),
    'trimmed': (lambda g: g.trimmed(before=float(np.median(EV[2])), keep_last=2), N, T_LAST),
    'without': (lambda g: g.without(nodes=[3, 17], eids=EV[3][:5]), N, T_LAST),
    'renumbered': (lambda g: g.renumbered(None, g._host_tcsr()[3].copy()), N, T_LAST),
}
KEEPS_MT = {'extended': False, 'extended-grown': False, 'widened': False, 'trimmed': True, 'without': True, 'renumbered': True}


def parent():
    from www2023tiger_amd.data.graph import Graph
    g = Graph.from_arrays(*EV, max_node_id=N - 1, strategy='recent_edges', seed=3)
    g.alpha = 0.25
    return g


@pytest.mark.parametrize('name', list(CHILDREN))
def test_a_child_carries_its_parent_over(name):
    derive, num_node, t_last = CHILDREN[name]
    g0 = parent()
    assert g0._dev is None and g0._time_ordered and g0._t_last == T_LAST
    before = [a.copy() for a in g0._host_tcsr()]
    sentinel = np.arange(3)
    g0._mt = sentinel
    g1 = derive(g0)
    assert g1 is not g0 and g1._dev is None and g1.num_node == num_node
    assert (g1.strategy, g1.seed, g1.alpha) == (g0.strategy, g0.seed, g0.alpha) == ('recent_edges', 3, 0.25)
    assert g1.rng is g0.rng
    assert g1._time_ordered is g0._time_ordered
    assert g1._t_last == t_last >= g0._t_last == T_LAST
    assert g1.serial != g0.serial
    if KEEPS_MT[name]:
        assert g1._mt is sentinel
    else:
        assert g1._mt is None
    assert g0._mt is sentinel
    g1._host_tcsr()  # (the child's host view is built from the parent's: that reads them too)
    for a, b in zip(g0._host_tcsr(), before):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
