"""tg_involved_list_host (the host twin of the involved-list entry) against the numpy reference of tests/_involved_ref.py,
exactly: listed ids, count, the bits of tmin and the bitmap afterwards; the argument errors of both entries (returned
before any launch, so they need no GPU); the workspace bound; the keywords of the evaluation functions.  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import _involved_ref as R

KS = (1, 5, 10, 17, 64)
QS = (0, 1, 3, 64, 65, 257)
STRATEGIES = ('recent_edges', 'recent_nodes')


def host_graph(name, strategy):
    from www2023tiger_amd.data.graph import Graph
    ev = R.events(name)
    return Graph.from_arrays(ev['src'], ev['dst'], ev['ts'], ev['eids'], strategy=strategy, max_node_id=ev['n_nodes'] - 1,
                             device='cpu')


def check_case(graph, name, K, L, strategy, Q, device='cpu'):
    """one (graph, K, layers, strategy, Q) against the reference for the three up-to-date states; -> the listed ids per
    state (for a caller that compares two implementations)"""
    from www2023tiger_amd import hip_ops
    ev = R.events(name)
    nid, ts = R.queries(ev, Q)
    involved = R.reference(name, ev, nid, ts, K, L, strategy)
    got_all = {}
    for state, upto in R.uptodate_states(ev['n_nodes']).items():
        ids, count, tmin, after = R.expected(involved, ts, upto)
        bm = torch.from_numpy(R.to_bitmap(upto)).to(device)
        out = hip_ops.involved_list(graph, torch.from_numpy(nid).to(device), torch.from_numpy(ts).to(device), K, L, bm,
                                    strategy=strategy)
        what = f'{name} K={K} L={L} {strategy} Q={Q} uptodate={state}'
        n = int(out['count'].item())
        assert n == count, what
        np.testing.assert_array_equal(out['ids'][:n].cpu().numpy(), ids, err_msg=what)
        np.testing.assert_array_equal(R.from_bitmap(bm.cpu().numpy(), ev['n_nodes']), after, err_msg=what)
        if Q:
            assert out['tmin'].cpu().numpy().view(np.uint32)[0] == np.array([tmin]).view(np.uint32)[0], what
        if state == 'full':
            assert n == 0, what
        got_all[state] = out['ids'][:n].cpu().numpy()
    return got_all


@pytest.mark.parametrize('strategy', STRATEGIES)
@pytest.mark.parametrize('L', (1, 2))
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('name', list(R.GRAPHS))
def test_host_twin_equals_the_reference(name, K, L, strategy):
    g = host_graph(name, strategy)
    for Q in QS:
        check_case(g, name, K, L, strategy, Q)


def test_full_bitmap_lists_nothing_and_leaves_the_list_untouched():
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import lib, ptr
    ev = R.events('hand65')
    g = host_graph('hand65', 'recent_edges')
    h = g._host_tcsr()
    tc = _lib.TgTcsr(g.num_node, len(h[1]), *(ptr(a) for a in h))
    nid, ts = R.queries(ev, 64)
    bm = R.to_bitmap(np.ones(65, bool))
    before = bm.copy()
    lst = np.full(65, -77, np.int64)
    count, tmin = np.full(1, -5, np.int32), np.full(1, np.nan, np.float32)
    rc = lib.tg_involved_list_host(C.byref(tc), 64, ptr(nid), ptr(ts), 10, 2, 0, ptr(bm), 65, ptr(lst), ptr(count), ptr(tmin))
    assert rc == 0 and count[0] == 0 and (lst == -77).all() and (bm == before).all()
    assert tmin[0] == np.float32(ts.min())
    # Q == 0: the count alone is written
    count[0], tmin[0] = -5, np.nan
    rc = lib.tg_involved_list_host(C.byref(tc), 0, None, None, 10, 2, 0, ptr(bm), 0, None, ptr(count), ptr(tmin))
    assert rc == 0 and count[0] == 0 and np.isnan(tmin[0]) and (bm == before).all()


def test_the_float32_case_tells_rounded_from_unrounded_hop2_times():
    """the hand-made graphs hold a neighbour time float32 cannot represent with another event of that neighbour between
    the rounded and the unrounded value: the second hop at the float32 time (what the collator samples) must not see
    node 3, a search at the float64 time would"""
    ev = R.events('hand64')
    og = R.oracle_graph(ev, 'recent_edges')
    nid, ts = np.array([1], np.int64), np.array([R.F32_QUERY_T])
    l_n, _, l_t, _ = og.sample_temporal_neighbor(nid, ts, 5, strategy='recent_edges')
    assert l_n[0, -1] == 2 and float(l_t[0, -1]) == 2.0 ** 27 and float(l_t[0, -1]) <= R.F32_BETWEEN < R.F32_T
    rounded = R.numpy_involved(og, nid, ts, 5, 2, 'recent_edges')
    unrounded = R.numpy_involved(og, nid, ts, 5, 2, 'recent_edges', round_hop2=False)
    assert 3 not in rounded and 3 in unrounded
    got = check_case(host_graph('hand64', 'recent_edges'), 'hand64', 5, 2, 'recent_edges', 1)
    assert 3 not in got['empty'] and 2 in got['empty']


def test_queries_hold_the_edge_cases():
    ev = R.events('hand129')
    nid, ts = R.queries(ev, 64)
    q = list(zip(nid.tolist(), ts.tolist()))
    assert (0, ev['ts'].max() + 1.0) in q and 128 in nid and R.ISOLATED in nid        # pad id, last node, no events at all
    assert any(t == ev['ts'][0] for _, t in q)                                       # nothing before the first event
    k = len(ev['ts']) // 2
    assert (int(ev['src'][k]), float(ev['ts'][k])) in q                              # a time equal to an event time
    assert len(set(q)) < len(q)                                                      # a query twice
    og = R.oracle_graph(ev, 'recent_edges')
    lo, hi = og.find_before(int(ev['src'][k]), float(ev['ts'][k]))
    assert hi < og.indptr[int(ev['src'][k]) + 1] and og.ts[hi] == ev['ts'][k]        # the strict cut leaves that event out


def _tcsr(g):
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import ptr
    h = g._host_tcsr()
    return _lib.TgTcsr(g.num_node, len(h[1]), *(ptr(a) for a in h)), h


def test_argument_errors_of_both_entries():
    """every refusal comes back before anything is launched or written: the device entry is called here with HOST
    pointers, which it never dereferences on these paths"""
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import lib, ptr
    g = host_graph('hand65', 'recent_edges')
    tc, _keep = _tcsr(g)
    n = g.num_node
    nid, ts = R.queries(R.events('hand65'), 3)
    bm, lst = R.to_bitmap(np.zeros(n, bool)), np.zeros(n, np.int64)
    count, tmin = np.zeros(1, np.int32), np.zeros(1, np.float32)
    ws = np.zeros(int(lib.tg_involved_list_workspace_bytes(n, 3, 10, 2)) + 64, np.uint8)
    wp = (ptr(ws) + 15) & ~15

    def host(Q=3, nids=ptr(nid), t=ptr(ts), K=10, L=2, strategy=0, upto=ptr(bm), cap=n, out=ptr(lst), cnt=ptr(count), tm=ptr(tmin)):
        return lib.tg_involved_list_host(C.byref(tc), Q, nids, t, K, L, strategy, upto, cap, out, cnt, tm)

    def device(Q=3, nids=ptr(nid), t=ptr(ts), K=10, L=2, strategy=0, upto=ptr(bm), cap=n, out=ptr(lst), cnt=ptr(count), tm=ptr(tmin),
               w=wp, wb=len(ws) - 16):
        return lib.tg_involved_list(C.byref(tc), Q, nids, t, K, L, strategy, upto, cap, out, cnt, tm, w, wb, None)

    assert host() == _lib.TG_OK
    for f in (host, device):
        assert f(strategy=2) == _lib.TG_EUNSUPPORTED
        for bad in (dict(K=0), dict(K=_lib.TG_INVOLVED_MAX_K + 1), dict(L=0), dict(L=3), dict(strategy=-1), dict(strategy=3),
                    dict(Q=-1), dict(nids=None), dict(t=None), dict(upto=None), dict(out=None), dict(cnt=None), dict(tm=None),
                    dict(cap=min(3 * (1 + 10 + 100), n) - 1)):
            assert f(**bad) == _lib.TG_EINVAL, (f.__name__, bad)
    assert device(w=None) == _lib.TG_EINVAL
    assert device(wb=int(lib.tg_involved_list_workspace_bytes(n, 3, 10, 2)) - 1) == _lib.TG_EINVAL
    assert host(cap=3 * (1 + 10), L=1) == _lib.TG_OK and host(cap=3 * (1 + 10) - 1, L=1) == _lib.TG_EINVAL
    out_of_range = np.array([1, n, 2], np.int64)
    assert host(nids=ptr(out_of_range)) == _lib.TG_EINVAL
    assert lib.tg_involved_list_host(None, 3, ptr(nid), ptr(ts), 10, 2, 0, ptr(bm), n, ptr(lst), ptr(count), ptr(tmin)) == _lib.TG_EINVAL


def test_python_wrapper_refusals():
    from www2023tiger_amd import hip_ops
    g = host_graph('hand65', 'recent_edges')
    nid, ts = (torch.from_numpy(a) for a in R.queries(R.events('hand65'), 3))
    bm = hip_ops.new_bitmap(65, 'cpu')
    with pytest.raises(NotImplementedError):
        hip_ops.involved_list(g, nid, ts, 10, 1, bm, strategy='uniform')
    with pytest.raises(ValueError):
        hip_ops.involved_list(g, torch.tensor([1, 65]), ts[:2], 10, 1, bm)
    with pytest.raises(ValueError):
        hip_ops.involved_list(g, nid, ts, 10, 1, bm[:1])
    with pytest.raises(ValueError):
        hip_ops.involved_list(g, nid, ts, 65, 1, bm)
    assert not bm.any()


def test_symbols_and_abi_version():
    from www2023tiger_amd._lib import lib
    for name in ('tg_involved_list_workspace_bytes', 'tg_involved_list', 'tg_involved_list_host'):
        assert getattr(lib, name) is not None
    assert lib.tg_abi_version() == 9


@pytest.mark.parametrize('K', (10, 20))
@pytest.mark.parametrize('L', (1, 2))
def test_workspace_has_no_term_in_the_slots(K, L):
    """the memory condition: at most 2 bytes per node + 16 bytes per hop-1 slot + 64 KiB - and nothing in Q K^2"""
    from www2023tiger_amd._lib import lib
    n_nodes, Q = 10 ** 4, 10 ** 5
    nbytes = int(lib.tg_involved_list_workspace_bytes(n_nodes, Q, K, L))
    assert 0 < nbytes <= 2 * n_nodes + 16 * Q * K + 65536
    assert nbytes < Q * K * K                                       # (no hop-2 array of even one byte per slot fits)
    assert nbytes == int(lib.tg_involved_list_workspace_bytes(n_nodes, 10 * Q, K, L))


def test_evaluation_functions_keep_restart_mode_and_gain_lazy_restarts():
    from www2023tiger_amd import eval_utils
    for f in (eval_utils.eval_edge_ranking, eval_utils.eval_recommendation):
        p = inspect.signature(f).parameters
        assert p['restart_mode'].default is False and p['lazy_restarts'].default is False
        assert p['uptodate_nodes'].default is None
