"""The snapshot-refresh kernels on the GPU (tg_catalogue_dirty, tg_catalogue_merge, tg_bitmap_mark_degree_diff), exactly:
device entry against host twin against the numpy reference of tests/_refresh_ref.py on the cases of
tests/test_snapshot_refresh_host.py; guard values behind every output; a short workspace; more than one scan tile with a
partial last tile (C = 2 049)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _involved_ref as R
import _refresh_ref as F
from test_snapshot_refresh_host import (CS, DS, KS, MERGE_CS, STRATEGIES, age_bound, check_degree_diff, check_dirty,
                                        check_merge, host_graph, merge_inputs, run_dirty)

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


def dev_graph(name, strategy):
    from www2023tiger_amd.data.graph import Graph
    ev = R.events(name)
    return Graph.from_arrays(ev['src'], ev['dst'], ev['ts'], ev['eids'], strategy=strategy, max_node_id=ev['n_nodes'] - 1,
                             device=dev())


@pytest.mark.parametrize('strategy', STRATEGIES)
@pytest.mark.parametrize('L', (1, 2))
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('name', F.GRAPH_NAMES)
def test_dirty_device_entry_equals_reference_and_host_twin(name, K, L, strategy):
    g, h = dev_graph(name, strategy), host_graph(name, strategy)
    for Cn in CS:
        got = check_dirty(g, name, K, L, strategy, Cn, device=dev())
        want = check_dirty(h, name, K, L, strategy, Cn)
        for state in got:
            np.testing.assert_array_equal(got[state][0], want[state][0], err_msg=f'{name} C={Cn} {state}')
            np.testing.assert_array_equal(got[state][1], want[state][1], err_msg=f'{name} C={Cn} {state}')
            assert got[state][2] == want[state][2]
    check_dirty(g, name, K, L, strategy, 65, device=dev(), uniform_time=True)
    check_dirty(g, name, K, L, strategy, 65, device=dev(), max_age=age_bound(name), states=('empty', 'half'))


def test_float32_hop2_and_age_boundary_on_the_device():
    g = dev_graph('hand64', 'recent_edges')
    ids, t_row = np.array([1], np.int64), np.array([R.F32_QUERY_T])
    for v, want in ((3, 0), (2, 1), (1, 1)):
        touched = np.zeros(64, bool)
        touched[v] = True
        assert run_dirty(g, ids, t_row, 5, 2, 'recent_edges', touched, R.F32_QUERY_T + 1, device=dev())[2][0] == want, v
    none = np.zeros(64, bool)
    ids, t_row = np.array([7, 8, 9], np.int64), np.array([0.0, 10.0, 50.0])
    above = float(np.nextafter(50.0, np.inf))
    assert run_dirty(g, ids, t_row, 2, 1, 'recent_edges', none, 50.0, 50.0, device=dev())[2] == (0, 0)
    rank, cols, count = run_dirty(g, ids, t_row, 2, 1, 'recent_edges', none, above, 50.0, device=dev())
    assert count == (1, 1) and cols.tolist() == [0] and rank.tolist() == [0, -1, -1]


@pytest.mark.parametrize('strategy', STRATEGIES)
def test_dirty_guards_short_workspace_and_two_tiles(strategy):
    """C = 2 049 (two scan tiles, the last one holding one row), called through the C ABI: nothing is written behind rank
    [C], cols [C] or count [2]; a workspace one byte short is refused before any launch"""
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    name, K, L, Cn, G = 'hand129', 10, 2, 2049, 64
    ev = R.events(name)
    g = dev_graph(name, strategy)
    ids, t_row = F.catalogue(ev, Cn)
    touched = F.touched_states(129)['half']
    t_new = float(ev['ts'].max()) + 20.0
    age = 2.0 ** 27   # (rows touched, rows old, rows both and rows neither; the one row of the last tile is dirty)
    want = F.dirty(name, strategy, K, L, ids, t_row, touched, t_new, age)
    d_ids, d_t = torch.from_numpy(ids).to(dev()), torch.from_numpy(t_row).to(dev())
    bm = torch.from_numpy(R.to_bitmap(touched)).to(dev())
    rank = torch.full((Cn + G,), -77, dtype=torch.int32, device=dev())
    cols = torch.full((Cn + G,), -77, dtype=torch.int32, device=dev())
    count = torch.full((2 + G,), -77, dtype=torch.int32, device=dev())
    need = int(lib.tg_catalogue_dirty_workspace_bytes(Cn))
    ws = torch.full((need + G,), 0x5a, dtype=torch.uint8, device=dev())
    args = (C.byref(g.tcsr), Cn, ptr(d_ids), ptr(d_t), 0.0, K, L, STRATEGIES.index(strategy), ptr(bm),
            t_new, age, ptr(rank), ptr(cols), ptr(count))
    assert lib.tg_catalogue_dirty(*args, ptr(ws), need - 1, stream_ptr(dev())) == _lib.TG_EWORKSPACE
    assert (rank == -77).all() and (count == -77).all()
    assert lib.tg_catalogue_dirty(*args, ptr(ws), need, stream_ptr(dev())) == _lib.TG_OK
    n = want['count'][0]
    assert 0 < want['count'][1] < n < Cn and want['rank'][2048] == n - 1
    assert count[:2].tolist() == list(want['count'])
    np.testing.assert_array_equal(rank[:Cn].cpu().numpy(), want['rank'])
    np.testing.assert_array_equal(cols[:n].cpu().numpy(), want['cols'])
    assert (cols[n:] == -77).all() and (rank[Cn:] == -77).all() and (count[2:] == -77).all() and (ws[need:] == 0x5a).all()
    # C == 0: count alone
    count[:] = -77
    assert lib.tg_catalogue_dirty(C.byref(g.tcsr), 0, None, None, 0.0, K, L, 0, None, t_new, float('nan'), None, None, ptr(count),
                                  None, 0, stream_ptr(dev())) == _lib.TG_OK
    assert count[:2].tolist() == [0, 0] and (count[2:] == -77).all()


@pytest.mark.parametrize('with_nb', (False, True))
@pytest.mark.parametrize('with_P', (False, True))
@pytest.mark.parametrize('d', DS)
def test_merge_device_entry_equals_the_reference(d, with_P, with_nb):
    for Cn in MERGE_CS:
        for n_new in sorted({0, Cn // 3, Cn}):
            for K in (1, 10):
                check_merge(Cn, d, K, n_new, with_P, with_nb, device=dev())
    check_merge(65, d, 64, 20, with_P, with_nb, t_old_scalar=True, device=dev())


@pytest.mark.parametrize('d,K', [(4, 1), (8, 10), (172, 10), (172, 64)])
def test_merge_guards(d, K):
    """all four outputs with guard rows behind row C - 1: rows past C are never stored; device == host twin"""
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    Cn, n_new, G = 2049, 700, 8
    t = merge_inputs(Cn, d, K, n_new)
    dv = {k: torch.from_numpy(v).to(dev()) for k, v in t.items()}
    h = torch.full((Cn + G, d), -7.0, dtype=torch.float32, device=dev())
    P = torch.full((Cn + G, d), -7.0, dtype=torch.float32, device=dev())
    nb = torch.full((Cn + G, K), -7, dtype=torch.int64, device=dev())
    tr = torch.full((Cn + G,), -7.0, dtype=torch.float64, device=dev())
    rc = lib.tg_catalogue_merge(Cn, n_new, d, K, ptr(dv['rank']), ptr(dv['h_old']), ptr(dv['h_new']), ptr(h), ptr(dv['P_old']),
                                ptr(dv['P_new']), ptr(P), ptr(dv['nb_old']), ptr(dv['nb_new']), ptr(nb), ptr(dv['t_old']), 0.0, 55.5,
                                ptr(tr), stream_ptr(dev()))
    assert rc == _lib.TG_OK
    np.testing.assert_array_equal(h[:Cn].cpu().numpy().view(np.uint32), F.merge(t['rank'], t['h_old'], t['h_new']).view(np.uint32))
    np.testing.assert_array_equal(P[:Cn].cpu().numpy().view(np.uint32), F.merge(t['rank'], t['P_old'], t['P_new']).view(np.uint32))
    np.testing.assert_array_equal(nb[:Cn].cpu().numpy(), F.merge(t['rank'], t['nb_old'], t['nb_new']))
    np.testing.assert_array_equal(tr[:Cn].cpu().numpy(), F.merge_times(t['rank'], t['t_old'], 55.5))
    assert (h[Cn:] == -7).all() and (P[Cn:] == -7).all() and (nb[Cn:] == -7).all() and (tr[Cn:] == -7).all()


@pytest.mark.parametrize('name', ('hand64', 'hand65', 'hand129', 'stream76'))
def test_degree_diff_device_entry_equals_the_reference(name):
    check_degree_diff(name, device=dev())
