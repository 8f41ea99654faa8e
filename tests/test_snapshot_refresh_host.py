"""The host twins of the snapshot-refresh entries (tg_catalogue_dirty_host, tg_catalogue_merge_host,
tg_bitmap_mark_degree_diff_host) against the numpy reference of tests/_refresh_ref.py, exactly; the argument errors of
all six entries (returned before any launch, so they need no GPU); the workspace bound.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import _involved_ref as R
import _refresh_ref as F

KS = (1, 2, 10, 64)
CS = (0, 1, 63, 64, 65, 2047, 2048, 2049)
STRATEGIES = ('recent_edges', 'recent_nodes')
DS = (4, 8, 172)


def host_graph(name, strategy):
    from www2023tiger_amd.data.graph import Graph
    ev = R.events(name)
    return Graph.from_arrays(ev['src'], ev['dst'], ev['ts'], ev['eids'], strategy=strategy, max_node_id=ev['n_nodes'] - 1,
                             device='cpu')


def age_bound(name):
    """a max_age with rows on both sides of it: half the span of the graph's times (rows are refreshed 20 after the end)"""
    return float(R.events(name)['ts'].max()) / 2 + 20.0


def run_dirty(graph, ids, t_row, K, L, strategy, touched, t_new, max_age=None, device='cpu'):
    """hip_ops.catalogue_dirty on numpy inputs -> (rank, cols[:n], (n_dirty, n_by_age)) as numpy / ints"""
    from www2023tiger_amd import hip_ops
    bm = torch.from_numpy(R.to_bitmap(touched)).to(device)
    tr = t_row if np.isscalar(t_row) else torch.from_numpy(np.asarray(t_row, np.float64)).to(device)
    out = hip_ops.catalogue_dirty(graph, torch.from_numpy(np.asarray(ids, np.int64)).to(device), tr, K, L, bm, t_new,
                                  max_age=max_age, strategy=strategy)
    n, n_age = (int(x) for x in out['count'].cpu().numpy())
    return out['rank'].cpu().numpy(), out['cols'][:n].cpu().numpy(), (n, n_age)


def check_dirty(graph, name, K, L, strategy, Cn, device='cpu', states=None, uniform_time=False, max_age=None):
    """one (graph, K, layers, strategy, C) against the reference for every touched state -> {state: (rank, cols, count)}"""
    ev = R.events(name)
    ids, t_row = F.catalogue(ev, Cn, uniform_time)
    t_new = float(ev['ts'].max()) + 20.0
    got_all = {}
    for state, touched in F.touched_states(ev['n_nodes']).items():
        if states is not None and state not in states:
            continue
        want = F.dirty(name, strategy, K, L, ids, t_row, touched, t_new, max_age)
        rank, cols, count = run_dirty(graph, ids, t_row, K, L, strategy, touched, t_new, max_age, device)
        what = f'{name} K={K} L={L} {strategy} C={Cn} touched={state} uniform={uniform_time} max_age={max_age}'
        assert count == want['count'], what
        np.testing.assert_array_equal(rank, want['rank'], err_msg=what)
        np.testing.assert_array_equal(cols, want['cols'], err_msg=what)
        if state == 'empty' and max_age is None:
            assert count == (0, 0), what
        if state == 'full':
            assert count[0] == Cn, what
        if state == 'empty' and max_age is not None and Cn >= 63:
            assert 0 < count[0] == count[1] < Cn, what   # by age alone, and not every row
        got_all[state] = (rank, cols, count)
    return got_all


@pytest.mark.parametrize('strategy', STRATEGIES)
@pytest.mark.parametrize('L', (1, 2))
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('name', F.GRAPH_NAMES)
def test_dirty_host_twin_equals_the_reference(name, K, L, strategy):
    g = host_graph(name, strategy)
    for Cn in CS:
        check_dirty(g, name, K, L, strategy, Cn)
    check_dirty(g, name, K, L, strategy, 65, uniform_time=True)                # t_row = None: one time for all rows
    check_dirty(g, name, K, L, strategy, 65, max_age=age_bound(name), states=('empty', 'half'))


def test_catalogue_holds_the_edge_cases():
    ev = R.events('hand129')
    ids, t_row = F.catalogue(ev, 2049)
    assert 0 in ids[:63] and 128 in ids[:63] and R.ISOLATED in ids[:63]
    assert len(set(zip(ids.tolist(), t_row.tolist()))) < len(ids)             # duplicates
    k = len(ev['ts']) // 2
    assert (int(ev['src'][k]), float(ev['ts'][k])) in set(zip(ids[:63].tolist(), t_row[:63].tolist()))  # an event's time
    assert (int(ev['src'][k]), float(ev['ts'][0])) in set(zip(ids[:63].tolist(), t_row[:63].tolist()))  # before the first


def test_the_reference_counts_of_the_issue_table():
    """endpoints of the last event / of the last five events on hand129, all 129 ids: the counts the issue states, from the
    reference and from the host twin"""
    ev = R.events('hand129')
    t = float(ev['ts'].max()) + 1.0
    table = {(2, 1): (5, 19), (10, 1): (12, 38), (2, 2): (13, 39), (10, 2): (37, 91)}
    for strategy in STRATEGIES:
        g = host_graph('hand129', strategy)
        for (K, L), (one, five) in table.items():
            for n_ev, want in ((1, one), (5, five)):
                touched = np.zeros(129, bool)
                touched[ev['src'][-n_ev:]] = touched[ev['dst'][-n_ev:]] = True
                assert F.dirty('hand129', strategy, K, L, np.arange(129), t, touched, t)['count'][0] == want, (strategy, K, L, n_ev)
                assert run_dirty(g, np.arange(129), t, K, L, strategy, touched, t)[2][0] == want, (strategy, K, L, n_ev)


def test_the_float32_hop2_case():
    """hand_events: the second hop of the slot (2, float32(F32_T)) of a query of node 1 must not see node 3 - a touched
    node 3 leaves the row clean, a touched node 2 makes it dirty"""
    g = host_graph('hand64', 'recent_edges')
    ids, t_row = np.array([1], np.int64), np.array([R.F32_QUERY_T])
    for v, want in ((3, 0), (2, 1), (1, 1)):
        touched = np.zeros(64, bool)
        touched[v] = True
        ref = F.dirty('hand64', 'recent_edges', 5, 2, ids, t_row, touched, R.F32_QUERY_T + 1)
        rank, cols, count = run_dirty(g, ids, t_row, 5, 2, 'recent_edges', touched, R.F32_QUERY_T + 1)
        assert count[0] == want == ref['count'][0], v
    assert 3 in R.numpy_involved(F.oracle_graph('hand64', 'recent_edges'), ids, t_row, 5, 2, 'recent_edges', round_hop2=False)


def test_an_event_at_the_row_time_does_not_count():
    """strict cut: a row embedded at an event's own time does not read that event's neighbour"""
    ev = R.events('hand129')
    g = host_graph('hand129', 'recent_edges')
    u, v, t = int(ev['src'][-1]), int(ev['dst'][-1]), float(ev['ts'][-1])   # the last event: (128, 6) and nothing after it
    touched = np.zeros(129, bool)
    touched[v] = True
    for t_row, want in ((t, 0), (np.nextafter(t, np.inf), 1)):
        ref = F.dirty('hand129', 'recent_edges', 1, 1, [u], [t_row], touched, t + 1)
        _, _, count = run_dirty(g, [u], [t_row], 1, 1, 'recent_edges', touched, t + 1)
        assert count[0] == want == ref['count'][0]


def test_max_age_boundary():
    g = host_graph('hand65', 'recent_edges')
    none = np.zeros(65, bool)
    ids = np.array([7, 8, 9], np.int64)
    t_row = np.array([0.0, 10.0, 50.0])
    above = float(np.nextafter(50.0, np.inf))
    # ages 50, 40, 0: equal to max_age is clean
    assert run_dirty(g, ids, t_row, 2, 1, 'recent_edges', none, 50.0, 50.0)[2] == (0, 0)
    # the next float64 above it is dirty
    rank, cols, count = run_dirty(g, ids, t_row, 2, 1, 'recent_edges', none, above, 50.0)
    assert count == (1, 1) and cols.tolist() == [0] and rank.tolist() == [0, -1, -1]
    assert F.dirty('hand65', 'recent_edges', 2, 1, ids, t_row, none, above, 50.0)['count'] == (1, 1)
    # max_age 0: every older row; a row that is touched as well is not counted as dirty by age alone
    one = none.copy()
    one[7] = True
    assert run_dirty(g, ids, t_row, 2, 1, 'recent_edges', one, 50.0, 0.0)[2] == (2, 1)
    assert run_dirty(g, ids, 50.0, 2, 1, 'recent_edges', none, above, 0.0)[2] == (3, 3)   # one time for all rows
    assert run_dirty(g, ids, t_row, 2, 1, 'recent_edges', none, 1e9, None)[2] == (0, 0)    # no bound: never by age


# ---- merge ---------------------------------------------------------------------------------------------------------------------
def merge_inputs(Cn, d, K, n_new, seed=0):
    rs = np.random.RandomState(seed + Cn + d)
    rank = np.full(Cn, -1, np.int32)
    rank[np.sort(rs.permutation(Cn)[:n_new])] = np.arange(n_new, dtype=np.int32)
    t = dict(rank=rank, h_old=rs.randn(Cn, d).astype(np.float32), h_new=rs.randn(n_new, d).astype(np.float32),
             P_old=rs.randn(Cn, d).astype(np.float32), P_new=rs.randn(n_new, d).astype(np.float32),
             nb_old=rs.randint(0, 1 << 40, (Cn, K)).astype(np.int64), nb_new=rs.randint(0, 1 << 40, (n_new, K)).astype(np.int64),
             t_old=rs.rand(Cn) * 100.0)
    return t


def check_merge(Cn, d, K, n_new, with_P, with_nb, t_old_scalar=False, device='cpu'):
    from www2023tiger_amd import hip_ops
    t = merge_inputs(Cn, d, K, n_new)
    dv = {k: torch.from_numpy(v).to(device) for k, v in t.items()}
    t_old = 3.25 if t_old_scalar else dv['t_old']
    kw = {}
    if with_P:
        kw.update(P_old=dv['P_old'], P_new=dv['P_new'])
    if with_nb:
        kw.update(nb_old=dv['nb_old'], nb_new=dv['nb_new'])
    h, P, nb, t_row = hip_ops.catalogue_merge(dv['rank'], n_new, dv['h_old'], dv['h_new'], t_old, 777.5, **kw)
    what = f'C={Cn} d={d} K={K} n_new={n_new} P={with_P} nb={with_nb}'
    np.testing.assert_array_equal(h.cpu().numpy().view(np.uint32), F.merge(t['rank'], t['h_old'], t['h_new']).view(np.uint32), what)
    assert (P is None) == (not with_P) and (nb is None) == (not with_nb)
    if with_P:
        np.testing.assert_array_equal(P.cpu().numpy().view(np.uint32), F.merge(t['rank'], t['P_old'], t['P_new']).view(np.uint32),
                                      what)
    if with_nb:
        np.testing.assert_array_equal(nb.cpu().numpy(), F.merge(t['rank'], t['nb_old'], t['nb_new']), what)
    np.testing.assert_array_equal(t_row.cpu().numpy(), F.merge_times(t['rank'], 3.25 if t_old_scalar else t['t_old'], 777.5), what)


MERGE_CS = (1, 63, 65, 2049)


@pytest.mark.parametrize('with_nb', (False, True))
@pytest.mark.parametrize('with_P', (False, True))
@pytest.mark.parametrize('d', DS)
def test_merge_host_twin_equals_the_reference(d, with_P, with_nb):
    for Cn in MERGE_CS:
        for n_new in sorted({0, Cn // 3, Cn}):
            for K in (1, 10):
                check_merge(Cn, d, K, n_new, with_P, with_nb)
    check_merge(65, d, 64, 20, with_P, with_nb, t_old_scalar=True)


# ---- degree difference ---------------------------------------------------------------------------------------------------------
def graph_pairs(name, device='cpu'):
    """(label, graph a, graph b) pairs: a graph and its extended / trimmed / without children, across a node-count change"""
    from www2023tiger_amd.data.graph import Graph
    ev = R.events(name)
    n = ev['n_nodes']
    cut = len(ev['ts']) - 5
    base = Graph.from_arrays(ev['src'][:cut], ev['dst'][:cut], ev['ts'][:cut], ev['eids'][:cut], strategy='recent_edges',
                             max_node_id=n - 1, device=device)
    ext = base.extended(ev['src'][cut:], ev['dst'][cut:], ev['ts'][cut:], ev['eids'][cut:])
    grown = base.extended(np.array([n, 7]), np.array([6, n]), np.array([ev['ts'][cut - 1]] * 2) + 1.0,
                          np.array([9001, 9002]), num_node=n + 1)   # ids 0 .. n: one more word when n is 64 or 128
    return [('extended', base, ext), ('trimmed', ext, ext.trimmed(keep_last=2)), ('without', ext, ext.without(nodes=[7, n - 1])),
            ('grown', base, grown), ('shrunk', grown, base), ('same', ext, ext)]


def check_degree_diff(name, device='cpu'):
    from www2023tiger_amd import hip_ops
    for label, a, b in graph_pairs(name, device):
        n = max(a.num_node, b.num_node)
        seeds = (np.zeros(n, bool), np.random.RandomState(n).rand(n) < 0.3)
        got = []
        for seed_bits in seeds:
            bm = torch.from_numpy(R.to_bitmap(seed_bits)).to(device)
            hip_ops.bitmap_mark_degree_diff(a, b, bm)
            got.append(bm.cpu().numpy())
        want = F.degree_diff(a._host_tcsr()[0], b._host_tcsr()[0])  # (after the device calls: the host view is a download)
        assert len(want) == n
        for seed_bits, words in zip(seeds, got):
            np.testing.assert_array_equal(R.from_bitmap(words, n), seed_bits | want, err_msg=f'{name} {label}')
            assert not R.from_bitmap(words, 64 * len(words))[n:].any(), f'{name} {label}: bits past the last id'
        if label == 'same':
            assert not want.any()
        else:
            assert want.any(), f'{name} {label}'
        if label == 'grown':
            assert want[n - 1] and n == a.num_node + 1


@pytest.mark.parametrize('name', ('hand64', 'hand65', 'hand129', 'stream76'))
def test_degree_diff_host_twin_equals_the_reference(name):
    check_degree_diff(name)


def test_degree_diff_word_edges():
    """64 -> 65 and 128 -> 129 node ids: the new id opens a bitmap word"""
    from www2023tiger_amd.data.graph import Graph
    from www2023tiger_amd import hip_ops
    for n in (64, 128):
        ev = R.hand_events(n)
        a = Graph.from_arrays(ev['src'], ev['dst'], ev['ts'], ev['eids'], strategy='recent_edges', max_node_id=n - 1, device='cpu')
        b = a.extended(np.array([n]), np.array([n - 1]), np.array([ev['ts'].max() + 1.0]), np.array([9001]), num_node=n + 1)
        bm = hip_ops.new_bitmap(n + 1, 'cpu')
        assert bm.numel() == n // 64 + 1
        hip_ops.bitmap_mark_degree_diff(a, b, bm)
        assert np.nonzero(R.from_bitmap(bm.numpy(), n + 1))[0].tolist() == [n - 1, n]
        with pytest.raises(ValueError):
            hip_ops.bitmap_mark_degree_diff(a, b, hip_ops.new_bitmap(n, 'cpu'))   # a bitmap over the smaller graph


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _tcsr(g):
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import ptr
    h = g._host_tcsr()
    return _lib.TgTcsr(g.num_node, len(h[1]), *(ptr(a) for a in h)), h


def test_argument_errors_of_the_dirty_entries():
    """every refusal comes back before anything is launched or written: the device entry is called here with HOST
    pointers, which it never dereferences on these paths"""
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import lib, ptr
    g = host_graph('hand65', 'recent_edges')
    tc, _keep = _tcsr(g)
    ids, t_row = F.catalogue(R.events('hand65'), 5)
    bm = R.to_bitmap(np.zeros(65, bool))
    rank, cols, count = np.full(5, -7, np.int32), np.full(5, -7, np.int32), np.full(2, -7, np.int32)
    need = int(lib.tg_catalogue_dirty_workspace_bytes(5))
    ws = np.zeros(need + 64, np.uint8)
    wp = (ptr(ws) + 15) & ~15
    nan = float('nan')

    def host(Cn=5, i=ptr(ids), tr=ptr(t_row), t_all=0.0, K=10, L=2, strategy=0, tb=ptr(bm), t_new=1e9, age=nan, r=ptr(rank),
             c=ptr(cols), n=ptr(count)):
        return lib.tg_catalogue_dirty_host(C.byref(tc), Cn, i, tr, t_all, K, L, strategy, tb, t_new, age, r, c, n)

    def device(Cn=5, i=ptr(ids), tr=ptr(t_row), t_all=0.0, K=10, L=2, strategy=0, tb=ptr(bm), t_new=1e9, age=nan, r=ptr(rank),
               c=ptr(cols), n=ptr(count), w=wp, wb=need):
        return lib.tg_catalogue_dirty(C.byref(tc), Cn, i, tr, t_all, K, L, strategy, tb, t_new, age, r, c, n, w, wb, None)

    assert host() == _lib.TG_OK and count.tolist() == [0, 0] and (rank == -1).all()
    rank[:], count[:] = -7, -7
    for f in (host, device):
        assert f(strategy=2) == _lib.TG_EUNSUPPORTED
        for bad in (dict(K=0), dict(K=_lib.TG_INVOLVED_MAX_K + 1), dict(L=0), dict(L=3), dict(strategy=-1), dict(strategy=3),
                    dict(Cn=-1), dict(Cn=2 ** 31), dict(i=None), dict(tb=None), dict(r=None), dict(c=None), dict(n=None),
                    dict(t_new=nan), dict(tr=None, t_all=nan), dict(age=-1.0)):
            assert f(**bad) == _lib.TG_EINVAL, (f.__name__, bad)
        assert (rank == -7).all() and (cols == -7).all() and (count == -7).all()
    assert device(w=None) == _lib.TG_EWORKSPACE
    assert device(wb=need - 1) == _lib.TG_EWORKSPACE
    assert device(w=wp + 8) == _lib.TG_EINVAL
    assert host(i=ptr(np.array([1, 2, 65, 3, 4], np.int64))) == _lib.TG_EINVAL
    assert lib.tg_catalogue_dirty_host(None, 5, ptr(ids), ptr(t_row), 0.0, 10, 2, 0, ptr(bm), 1e9, nan, ptr(rank), ptr(cols),
                                       ptr(count)) == _lib.TG_EINVAL
    # C == 0: the host twin zeroes count and needs no other array
    count[:] = -7
    assert host(Cn=0, i=None, tr=None, tb=None, r=None, c=None) == _lib.TG_OK and count.tolist() == [0, 0]


def test_argument_errors_of_the_merge_and_degree_entries():
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import lib, ptr
    t = merge_inputs(5, 8, 3, 2)
    out_h, out_P, out_nb, out_t = np.zeros((5, 8), np.float32), np.zeros((5, 8), np.float32), np.zeros((5, 3), np.int64), np.zeros(5)
    p = {k: ptr(v) for k, v in t.items()}
    for v in list(t.values()) + [out_h, out_P]:
        assert ptr(v) % 16 == 0

    def call(f, Cn=5, n_new=2, d=8, K=3, rank=p['rank'], ho=p['h_old'], hn=p['h_new'], hx=ptr(out_h), Po=p['P_old'], Pn=p['P_new'],
             Px=ptr(out_P), no=p['nb_old'], nn=p['nb_new'], nx=ptr(out_nb), to=p['t_old'], tx=ptr(out_t)):
        args = (Cn, n_new, d, K, rank, ho, hn, hx, Po, Pn, Px, no, nn, nx, to, 0.0, 9.0, tx)
        return f(*args) if f is lib.tg_catalogue_merge_host else f(*args, None)

    assert call(lib.tg_catalogue_merge_host) == _lib.TG_OK
    for f in (lib.tg_catalogue_merge_host, lib.tg_catalogue_merge):
        for bad in (dict(Cn=-1), dict(Cn=2 ** 31), dict(n_new=-1), dict(n_new=6), dict(d=0), dict(d=6), dict(K=-1), dict(rank=None),
                    dict(ho=None), dict(hn=None), dict(hx=None), dict(tx=None), dict(Po=None), dict(Pn=None), dict(Px=None),
                    dict(no=None), dict(nn=None), dict(nx=None), dict(K=0), dict(hx=ptr(out_h) + 4)):
            assert call(f, **bad) == _lib.TG_EINVAL, bad
    assert call(lib.tg_catalogue_merge_host, Po=None, Pn=None, Px=None, no=None, nn=None, nx=None, K=0) == _lib.TG_OK
    bad_rank = t['rank'].copy()
    bad_rank[bad_rank < 0] = 2
    assert call(lib.tg_catalogue_merge_host, rank=ptr(bad_rank)) == _lib.TG_EINVAL
    # degree difference
    g = host_graph('hand65', 'recent_edges')
    tc, _keep = _tcsr(g)
    bm = np.zeros(2, np.int64)
    for f in (lambda *a: lib.tg_bitmap_mark_degree_diff_host(*a), lambda *a: lib.tg_bitmap_mark_degree_diff(*a, None)):
        assert f(None, C.byref(tc), ptr(bm), 2) == _lib.TG_EINVAL
        assert f(C.byref(tc), None, ptr(bm), 2) == _lib.TG_EINVAL
        assert f(C.byref(tc), C.byref(tc), None, 2) == _lib.TG_EINVAL
        assert f(C.byref(tc), C.byref(tc), ptr(bm), 1) == _lib.TG_EINVAL
    assert lib.tg_bitmap_mark_degree_diff_host(C.byref(tc), C.byref(tc), ptr(bm), 2) == _lib.TG_OK and not bm.any()


def test_python_wrapper_refusals():
    from www2023tiger_amd import hip_ops
    g = host_graph('hand65', 'recent_edges')
    ids, t_row = (torch.from_numpy(a) for a in F.catalogue(R.events('hand65'), 3))
    bm = hip_ops.new_bitmap(65, 'cpu')
    with pytest.raises(NotImplementedError):
        hip_ops.catalogue_dirty(g, ids, t_row, 10, 1, bm, 1e9, strategy='uniform')
    for bad in (dict(ids=torch.tensor([1, 65, 2])), dict(bm=bm[:1]), dict(K=65), dict(L=3), dict(t_new=float('nan')),
                dict(max_age=-1.0), dict(max_age=float('nan')), dict(t_row=t_row[:2])):
        a = dict(ids=ids, t_row=t_row, K=10, L=1, bm=bm, t_new=1e9, max_age=None)
        a.update(bad)
        with pytest.raises(ValueError):
            hip_ops.catalogue_dirty(g, a['ids'], a['t_row'], a['K'], a['L'], a['bm'], a['t_new'], max_age=a['max_age'])
    rank = torch.tensor([-1, 0, -1], dtype=torch.int32)
    h_old, h_new = torch.zeros(3, 8), torch.ones(1, 8)
    for bad in (dict(rank=rank.long()), dict(n_new=4), dict(h_new=torch.ones(1, 4)), dict(h_old=torch.zeros(3, 6), h_new=torch.ones(1, 6)),
                dict(P_old=torch.zeros(3, 8)), dict(nb_new=torch.zeros(1, 2, dtype=torch.int64))):
        a = dict(rank=rank, n_new=1, h_old=h_old, h_new=h_new, P_old=None, P_new=None, nb_old=None, nb_new=None)
        a.update(bad)
        with pytest.raises(ValueError):
            hip_ops.catalogue_merge(a['rank'], a['n_new'], a['h_old'], a['h_new'], 0.0, 1.0, P_old=a['P_old'], P_new=a['P_new'],
                                    nb_old=a['nb_old'], nb_new=a['nb_new'])


def test_symbols_and_abi_version():
    from www2023tiger_amd._lib import lib
    for name in ('tg_catalogue_dirty_workspace_bytes', 'tg_catalogue_dirty', 'tg_catalogue_dirty_host', 'tg_catalogue_merge',
                 'tg_catalogue_merge_host', 'tg_bitmap_mark_degree_diff', 'tg_bitmap_mark_degree_diff_host'):
        assert getattr(lib, name) is not None
    assert lib.tg_abi_version() == 9


def test_workspace_is_linear_in_the_rows_alone():
    """one flag byte per row + 8 bytes per tile of 2 048 rows: no term in C K"""
    from www2023tiger_amd._lib import lib
    for Cn in (1, 2048, 2049, 10 ** 6):
        nbytes = int(lib.tg_catalogue_dirty_workspace_bytes(Cn))
        assert Cn <= nbytes <= Cn + 8 * ((Cn + 2047) // 2048) + 64
    assert int(lib.tg_catalogue_dirty_workspace_bytes(-1)) == 0 and int(lib.tg_catalogue_dirty_workspace_bytes(2 ** 31)) == 0
