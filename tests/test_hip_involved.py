"""tg_involved_list on the GPU, exactly: against the numpy reference of tests/_involved_ref.py, the host twin, and the flags
GraphCollator.collate_memory_nodes leaves for the same queries (the path the entry replaces); at the grid cap of its
one-wavefront-per-query launch and past it; on a graph past 65 536 nodes (the listing then takes its two-launch form)."""
import numpy as np
import pytest
import torch

import _cap_ref as CR
import _involved_ref as R
from test_involved_host import KS, QS, STRATEGIES, check_case, host_graph

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


def dev_graph(ev, strategy):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(ev['src'], ev['dst'], ev['ts'], ev['eids'], strategy=strategy, max_node_id=ev['n_nodes'] - 1,
                             device=dev())


def collator_flags(g, nid, ts, K, L):
    """the involved set as the path in use before lists it: collate_memory_nodes (slot arrays and all) + unique_compact"""
    from www2023tiger_amd.data.data_loader import GraphCollator
    _, _, comp = GraphCollator(g, K, L).collate_memory_nodes(torch.from_numpy(nid).to(dev()), torch.from_numpy(ts).to(dev()))
    return comp['ids'][:int(comp['count'].item())].cpu().numpy()


@pytest.mark.parametrize('strategy', STRATEGIES)
@pytest.mark.parametrize('L', (1, 2))
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('name', list(R.GRAPHS))
def test_device_entry_equals_reference_host_twin_and_collator(name, K, L, strategy):
    ev = R.events(name)
    g, h = dev_graph(ev, strategy), host_graph(name, strategy)
    for Q in QS:
        got = check_case(g, name, K, L, strategy, Q, device=dev())
        want = check_case(h, name, K, L, strategy, Q)
        for state in got:
            np.testing.assert_array_equal(got[state], want[state], err_msg=f'{name} Q={Q} {state}')
        if Q:
            nid, ts = R.queries(ev, Q)
            np.testing.assert_array_equal(got['empty'], collator_flags(g, nid, ts, K, L), err_msg=f'{name} Q={Q} collator')


def _both(g, h, nid, ts, K, L, strategy, upto):
    """device entry and host twin on the same inputs -> (ids, bitmap afterwards) of each, after comparing count and tmin"""
    from www2023tiger_amd import hip_ops
    out = []
    for graph, device in ((g, dev()), (h, 'cpu')):
        bm = torch.from_numpy(R.to_bitmap(upto)).to(device)
        o = hip_ops.involved_list(graph, torch.from_numpy(nid).to(device), torch.from_numpy(ts).to(device), K, L, bm,
                                  strategy=strategy)
        n = int(o['count'].item())
        out.append((o['ids'][:n].cpu().numpy(), bm.cpu().numpy(), o['tmin'].cpu().numpy().view(np.uint32)[0]))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2]
    return out[0]


# the marking launch: `flat_grid(Q, 4)` 256-thread workgroups, one wavefront per query
Q_AT = CR.FLAT_BLOCKS * CR.PER_WAVE
Q_PAST = Q_AT + 37


@pytest.mark.parametrize('strategy', STRATEGIES)
@pytest.mark.parametrize('Q', [Q_AT, Q_PAST], ids=['at-the-cap', 'past-the-cap'])
def test_at_and_past_the_grid_cap(Q, strategy):
    """K = 5, two layers: the wavefronts of the second pass mark as the first ones do"""
    assert (Q_AT, Q_PAST) == (16384, 16384 + 37)
    N, src, dst, ts_ev, eids = CR.small_graph()
    ev = dict(src=src, dst=dst, ts=ts_ev, eids=eids, n_nodes=N)
    nid, ts = CR.queries(N, Q, ts_ev[-1], seed=Q)
    # the last ten nodes have no event, so only a query reaches them - and only queries of the second pass ask for them: a
    # skipped second pass cannot hide behind the first
    nid[:Q_AT][nid[:Q_AT] >= N - 10] = 1
    if Q > Q_AT:
        nid[-10:] = np.arange(N - 10, N)
    assert not np.isin(np.arange(N - 10, N), np.concatenate([src, dst])).any()
    from www2023tiger_amd.data.graph import Graph
    h = Graph.from_arrays(src, dst, ts_ev, eids, strategy=strategy, max_node_id=N - 1, device='cpu')
    upto = np.zeros(N, bool)
    ids, bm, tmin = _both(dev_graph(ev, strategy), h, nid, ts, 5, 2, strategy, upto)
    assert tmin == np.array([np.float32(ts.min())]).view(np.uint32)[0]
    assert np.isin(np.arange(N - 10, N), ids).all() == (Q > Q_AT)
    if strategy == 'recent_edges':   # (the oracle's recent_nodes is a Python loop over 10^5 queries: the host twin stands in)
        want = R.numpy_involved(R.oracle_graph(ev, strategy), nid, ts, 5, 2, strategy)
        np.testing.assert_array_equal(ids, want)
        np.testing.assert_array_equal(R.from_bitmap(bm, N), np.isin(np.arange(N), want))


@pytest.mark.parametrize('strategy', STRATEGIES)
def test_graph_past_65536_nodes_lists_in_two_launches(strategy):
    """1 094 bitmap words: k_involved_pack / k_involved_emit, several 256-word blocks, a ragged last one"""
    n_nodes = 70000
    rs = np.random.RandomState(11)
    pool = np.unique(np.concatenate([rs.randint(1, n_nodes, 500), [n_nodes - 1, 65535, 65536, 16383, 16384]]))
    E = 3000
    ev = dict(src=pool[rs.randint(0, len(pool), E)].astype(np.int64), dst=pool[rs.randint(0, len(pool), E)].astype(np.int64),
              ts=np.sort(rs.randint(1, 500, E)).astype(np.float64), eids=np.arange(1, E + 1, dtype=np.int64), n_nodes=n_nodes)
    Q = 300
    nid = pool[rs.randint(0, len(pool), Q)].astype(np.int64)
    nid[:3] = [0, n_nodes - 1, 65536]
    ts = rs.randint(1, 520, Q).astype(np.float64)
    from www2023tiger_amd.data.graph import Graph
    h = Graph.from_arrays(ev['src'], ev['dst'], ev['ts'], ev['eids'], strategy=strategy, max_node_id=n_nodes - 1, device='cpu')
    want = R.numpy_involved(R.oracle_graph(ev, strategy), nid, ts, 5, 2, strategy)
    for upto in (np.zeros(n_nodes, bool), rs.rand(n_nodes) < 0.5):
        ids, bm, _ = _both(dev_graph(ev, strategy), h, nid, ts, 5, 2, strategy, upto)
        exp_ids, _, _, after = R.expected(want, ts, upto)
        np.testing.assert_array_equal(ids, exp_ids)
        np.testing.assert_array_equal(R.from_bitmap(bm, n_nodes), after)
    assert len(want) > 256 and want[-1] == n_nodes - 1


def test_second_call_lists_nothing():
    from www2023tiger_amd import hip_ops
    ev = R.events('stream76')
    g = dev_graph(ev, 'recent_edges')
    nid, ts = (torch.from_numpy(a).to(dev()) for a in R.queries(ev, 65))
    bm = hip_ops.new_bitmap(ev['n_nodes'], dev())
    first = hip_ops.involved_list(g, nid, ts, 10, 2, bm)
    assert int(first['count'].item()) > 0
    after = bm.clone()
    second = hip_ops.involved_list(g, nid, ts, 10, 2, bm)
    assert int(second['count'].item()) == 0 and torch.equal(bm, after)
    assert torch.equal(second['tmin'], first['tmin'])
