"""tg_trending_host and tg_fill_candidates_host (the host twins of the trending-candidate entries) and their Python fronts
against the numpy reference of tests/_trend_ref.py, array for array.  The argument errors of all four C entries come back
before any launch, so they need no GPU either.  The check_* functions take the device the tensors live on: 'cpu' runs the
host twins, tests/test_hip_trend.py runs the same cases through the kernels."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _trend_ref as R
import _walk_ref as W


def run_trending(N, ev, ref, t, T, device, what, window=None, among=None):
    """one call on `device` (and, off the CPU, the host twin as well) against the reference -> the reference's dict"""
    want = R.trending(ref, t, T, window, among)
    R.assert_same(R.library_trending(W.library_graph(N, ev, device), t, T, device, window, among), want, what)
    if str(device) != 'cpu':
        R.assert_same(R.library_trending(W.library_graph(N, ev, 'cpu'), t, T, 'cpu', window, among), want, what + ' (host twin)')
    return want


def run_fill(N, ev, ref, src, ts, cand, fill_ids, n_fill, device, what, **flags):
    want = R.fill(ref, src, ts, cand, fill_ids, n_fill, **flags)
    R.assert_same(R.library_fill(W.library_graph(N, ev, device), src, ts, cand, fill_ids, n_fill, device, **flags), want, what,
                  R.FILL_NAMES)
    if str(device) != 'cpu':
        R.assert_same(R.library_fill(W.library_graph(N, ev, 'cpu'), src, ts, cand, fill_ids, n_fill, 'cpu', **flags), want,
                      what + ' (host twin)', R.FILL_NAMES)
    return want


# ---- trending --------------------------------------------------------------------------------------------------------------
def check_among_sizes(M, device):
    """a random list of M ids, the same list permuted and reversed: one answer; every T; two windows"""
    N, ev, ref = R.wide_case()
    among = R.among_list(M, seed=M)
    t = float(ev[2].max()) / 2
    for T in R.TS:
        for window in (None, 60.0):
            want = run_trending(N, ev, ref, t, T, device, f'M={M} T={T} window={window}', window, among)
            for perm in (among[::-1], np.random.RandomState(T).permutation(among)):
                R.assert_same(R.library_trending(W.library_graph(N, ev, device), t, T, device, window, perm), want,
                              f'M={M} T={T}, permuted')
            assert 0 not in want['ids'][:want['n_valid'][0]]
            if M >= 15 and window is None:
                assert want['ids'][0] == 9 and want['n_distinct'][0] < M     # the hub leads; ids without entries are not listed
    if M == 4097:
        assert want['n_distinct'][0] > 64                                     # T < n_distinct and T > n_distinct both ran


@pytest.mark.parametrize('M', R.MS)
def test_trending_among_lists_of_every_size(M):
    check_among_sizes(M, 'cpu')


def check_windows(device):
    N, ev, ref = R.wide_case()
    among = R.among_list(2049, seed=7)
    seen = {}
    for name, t, window in R.windows():
        for am in (among, None):
            for T in (16, 2048):
                want = run_trending(N, ev, ref, t, T, device, f'{name} T={T} among={am is not None}', window, am)
        seen[name] = int(want['n_distinct'][0])
    assert seen['empty'] == 0 and seen['before-everything'] == 0 and seen['before-everything-window'] == 0
    assert seen['all'] == seen['wider-than-history'] >= seen['half'] > 0 and 0 < seen['on-events'] and 0 < seen['recent'] < seen['all']
    # both bounds ON an event time: the entries at t_lo count, the entries at t_hi do not
    _, t, window = [w for w in R.windows() if w[0] == 'on-events'][0]
    ts = ev[2]
    assert (ts == t).any() and (ts == t - window).any()
    total = R.trending(ref, t, 2048, window)['counts'].sum() + R.count(ref, 0, t - window, t)
    assert total == 2 * int(((ts >= t - window) & (ts < t)).sum())


def test_trending_windows():
    check_windows('cpu')


def check_ties(device):
    N, ev, among = R.tie_case()
    ref = W.WalkRef(N, *ev[:3])
    t = float(len(ev[0]) + 1)
    for T in (64, 2048):
        want = run_trending(N, ev, ref, t, T, device, f'ties T={T}', None, among)
        assert want['ids'][:3].tolist() == sorted(R.TIE_HEAVY) and want['counts'][:3].tolist() == [5, 5, 5]
        rest = [v for v in range(R.TIE_FIRST, R.TIE_FIRST + T) if v not in R.TIE_HEAVY][:T - 3]
        assert want['ids'][3:].tolist() == rest and (want['counts'][3:] == 2).all()      # ascending id decides inside the tie
        assert want['n_distinct'][0] == R.TIE_ITEMS
    at = {int(v): i for i, v in enumerate(among)}
    assert at[R.TIE_FIRST + 29] == R.TILE and at[R.TIE_FIRST + 30] == R.TILE - 1         # the picked ids straddle the tile edge
    run_trending(N, ev, ref, t, 64, device, 'ties, every node', None, None)


def test_trending_ties_across_a_tile_edge():
    check_ties('cpu')


def check_degrees(device):
    N, ev, among = R.degree_case()
    ref = W.WalkRef(N, *ev[:3])
    for t, window in ((290.0, None), (289.0, None), (288.0, 272.0), (17.0, 1.0), (17.0, 16.0), (18.0, 17.0), (289.0, 1.0), (1.0, None),
                      (2.0, None)):
        want = run_trending(N, ev, ref, t, 16, device, f'degrees t={t} window={window}', window, among)
        run_trending(N, ev, ref, t, 16, device, f'degrees t={t} window={window}, every node', window, None)
    assert want['ids'][:5].tolist() == [11, 12, 13, 14, 15] and want['counts'][:5].tolist() == [1] * 5    # t = 2: one entry each
    full = R.trending(ref, 290.0, 16, None, among)
    assert full['ids'][:5].tolist() == [15, 14, 13, 12, 11] and full['counts'][:5].tolist() == [289, 288, 17, 16, 1]


def test_trending_degrees_at_the_probe_rounds():
    check_degrees('cpu')


def check_derived_graphs(device):
    """Graph.trimmed(keep_last=8) and Graph.extended(batch) against the reference over the corresponding entries"""
    N, ev, ref = R.wide_case()
    t = float(ev[2].max()) + 1.0
    among = R.among_list(2049, seed=3)
    g = W.library_graph(N, ev, device)
    if str(device) != 'cpu':
        g.tcsr   # resident: trimmed and extended then run on the device
    for am in (None, among):
        for window in (None, 300.0):
            want = R.trending(ref.trimmed(8), t, 64, window, am)
            R.assert_same(R.library_trending(g.trimmed(keep_last=8), t, 64, device, window, am), want, 'trimmed')
            assert want['counts'].max() == 8 and not np.array_equal(want['ids'], R.trending(ref, t, 64, window, am)['ids'])
    cut = len(ev[0]) - 500
    old, new = tuple(a[:cut] for a in ev), tuple(a[cut:] for a in ev)
    parent = W.library_graph(N, old, device)
    if str(device) != 'cpu':
        parent.tcsr
    child = parent.extended(*(torch.from_numpy(a).to(device) for a in new))
    R.assert_same(R.library_trending(child, t, 64, device, 200.0, among), R.trending(ref, t, 64, 200.0, among), 'extended')
    R.assert_same(R.library_trending(parent, t, 64, device, 200.0, among),
                  R.trending(W.WalkRef(N, *old[:3]), t, 64, 200.0, among), 'the parent stays')


def test_trending_on_trimmed_and_extended_graphs():
    check_derived_graphs('cpu')


# ---- fill ------------------------------------------------------------------------------------------------------------------
def check_fill(Cn, T, device):
    N, ev, ref = R.wide_case()
    B = 24 if Cn >= 512 else 48
    src, ts, cand = R.fill_rows(B, Cn, seed=Cn + T)
    fill_ids, n_fill = R.fill_universe(T, seed=T)
    for flags in (dict(), dict(exclude_seen=True), dict(keep_self=True), dict(exclude_seen=True, keep_self=True)):
        want = run_fill(N, ev, ref, src, ts, cand, fill_ids, n_fill, device, f'C={Cn} T={T} {flags}', **flags)
        full = cand['n_valid'] >= Cn
        assert full.any() and (want['n_filled'][full] == 0).all()
        assert np.array_equal(want['ids'][full], cand['ids'][full]) and np.array_equal(want['counts'][full], cand['counts'][full])
        for i in range(B):
            nv = want['n_valid'][i]
            assert (want['ids'][i, nv:] == -7).all() and (want['counts'][i, nv:] == -7).all()      # not written
            new = want['ids'][i, cand['n_valid'][i]:nv]
            assert set(new.tolist()) <= set(fill_ids[:n_fill].tolist()) - {0} and len(set(want['ids'][i, :nv].tolist())) >= nv - 1
            if 'keep_self' not in flags:
                assert src[i] not in new
    return want


@pytest.mark.parametrize('T', R.FILL_TS)
@pytest.mark.parametrize('Cn', R.FILL_CS)
def test_fill_equals_the_reference(Cn, T):
    check_fill(Cn, T, 'cpu')


def check_fill_special(device):
    N, ev, ref = R.wide_case()
    t_max = float(ev[2].max()) + 1.0
    # the fill list wholly inside the row; the source in the list with and without keep_self; id 0 inside the list
    fill_ids = np.array([5, 0, 9, 17, 33, 450], np.int64)
    ids = np.full((3, 8), -7, np.int64)
    ids[0, :6] = (450, 33, 17, 9, 5, 7)
    ids[1, :2] = (7, 7)                                     # a caller-made row with a repeated id
    cand = dict(ids=ids, counts=np.full((3, 8), 3, np.int32), n_valid=np.array([6, 2, 0], np.int32))
    src, ts = np.array([1, 9, 450], np.int64), np.full(3, t_max)
    plain = run_fill(N, ev, ref, src, ts, cand, fill_ids, 6, device, 'special')
    assert plain['n_filled'].tolist() == [0, 4, 4] and plain['ids'][1, :7].tolist() == [7, 7, 5, 17, 33, 450, -7]
    assert plain['ids'][2, :5].tolist() == [5, 9, 17, 33, -7]
    kept = run_fill(N, ev, ref, src, ts, cand, fill_ids, 6, device, 'special keep_self', keep_self=True)
    assert kept['ids'][1, :7].tolist() == [7, 7, 5, 9, 17, 33, 450] and kept['ids'][2, :5].tolist() == [5, 9, 17, 33, 450]
    # a cold source gets exactly the first C admissible trending ids
    trend = R.trending(ref, t_max, 64)
    cold = dict(ids=np.zeros((1, 16), np.int64), counts=np.zeros((1, 16), np.int32), n_valid=np.zeros(1, np.int32))
    got = run_fill(N, ev, ref, np.array([450], np.int64), np.array([t_max]), cold, trend['ids'], int(trend['n_valid'][0]), device,
                   'cold', exclude_seen=True)
    assert got['ids'][0].tolist() == trend['ids'][:16].tolist() and got['n_filled'][0] == 16 and (got['counts'] == 0).all()
    # n_fill == 0, and below zero: nothing is appended
    for nf in (0, -3):
        none = run_fill(N, ev, ref, src, ts, cand, fill_ids, nf, device, f'n_fill={nf}')
        assert none['n_filled'].tolist() == [0, 0, 0] and np.array_equal(none['ids'], cand['ids'])


def test_fill_special_rows():
    check_fill_special('cpu')


def check_fill_sweep(n, device):
    N, ev, src, ts, fill_ids = R.sweep_fill_case(n)
    ref = W.WalkRef(N, *ev[:3])
    assert len(ref.prefix(W.SWEEP_S, ts[0])) == n and len(ref.t[W.SWEEP_S]) == n + 1      # one entry exactly at the query's time
    cand = dict(ids=np.full((1, 16), -7, np.int64), counts=np.full((1, 16), -7, np.int32), n_valid=np.zeros(1, np.int32))
    plain = run_fill(N, ev, ref, src, ts, cand, fill_ids, len(fill_ids), device, f'prefix {n}')
    seen = run_fill(N, ev, ref, src, ts, cand, fill_ids, len(fill_ids), device, f'prefix {n} exclude_seen', exclude_seen=True)
    assert plain['ids'][0, :7].tolist() == [W.SWEEP_X, 5, W.SWEEP_Y, 10, 11, 59, W.SWEEP_U]
    got = seen['ids'][0, :seen['n_valid'][0]].tolist()
    assert got[:2] == ([5, W.SWEEP_Y] if n else [W.SWEEP_X, 5]) and 5 in got              # the entry AT ts is not seen
    if n >= 257:
        assert got == [5, W.SWEEP_Y, W.SWEEP_U]                                           # X and the whole pool were seen


@pytest.mark.parametrize('n', W.SWEEP_PREFIXES)
def test_fill_exclude_seen_sweeps_the_whole_prefix(n):
    check_fill_sweep(n, 'cpu')


def check_fill_strides(device):
    N, ev, src, ts, fill_ids = R.stride_fill_case()
    ref = W.WalkRef(N, *ev[:3])
    B = len(src)
    cand = dict(ids=np.full((B, 2048), -7, np.int64), counts=np.full((B, 2048), -7, np.int32), n_valid=np.zeros(B, np.int32))
    cand['ids'][4, :40], cand['n_valid'][4] = fill_ids[5:2005:50], 40                     # a row that holds forty of them
    want = run_fill(N, ev, ref, src, ts, cand, fill_ids, 2048, device, 'strides', exclude_seen=True)
    assert want['n_filled'].tolist() == [2048, 2040, 2040, 2048, 2008]
    short = dict(ids=cand['ids'][:, :100].copy(), counts=cand['counts'][:, :100].copy(), n_valid=cand['n_valid'].copy())
    run_fill(N, ev, ref, src, ts, short, fill_ids, 2048, device, 'strides, C = 100', exclude_seen=True)


def test_fill_power_of_two_strides_fill_the_table():
    check_fill_strides('cpu')


# ---- fronts and symbols ----------------------------------------------------------------------------------------------------
def _tcsr(g):
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import ptr
    h = g._host_tcsr()
    return _lib.TgTcsr(g.num_node, len(h[1]), *(ptr(a) for a in h)), h


def test_symbols_cap_and_abi_version():
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import lib
    for name in ('tg_trending', 'tg_trending_host', 'tg_trending_workspace_bytes', 'tg_fill_candidates', 'tg_fill_candidates_host',
                 'tg_fill_candidates_lds_bytes'):
        assert getattr(lib, name) is not None
    assert lib.tg_abi_version() == 9 and _lib.TG_TREND_MAX == R.TREND_MAX
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'tiger_hip.h')).read()
    assert '#define TG_TREND_MAX 2048\n' in header


def test_lds_and_workspace_budgets():
    from www2023tiger_amd._lib import lib
    for T in (1, 256, 2048):
        n = int(lib.tg_fill_candidates_lds_bytes(T))
        assert 0 < n <= 64 * 1024 and n % 16 == 0, T
    assert int(lib.tg_fill_candidates_lds_bytes(2049)) == 0 and int(lib.tg_fill_candidates_lds_bytes(0)) == 0
    assert 4 * int(lib.tg_fill_candidates_lds_bytes(256)) <= 160 * 1024
    # 8 bytes per eligible node (whole tiles) plus the merge buffers: at T = 2 048 these are 17 / 256 of the keys
    for M in (0, 1, 2048, 2049, 10 ** 6, 10 ** 7):
        for T in (1, 256, 2048):
            tiles = max(1, -(-M // R.TILE))
            keys = tiles * R.TILE * 8
            ws = int(lib.tg_trending_workspace_bytes(M, T))
            assert keys <= ws <= keys + (keys * T // 2048 * 17) // 256 + 2 * T * 8 + 8 * tiles + 64, (M, T, ws)
            assert ws % 16 == 0
    assert int(lib.tg_trending_workspace_bytes(100, 2049)) == 0 and int(lib.tg_trending_workspace_bytes(-1, 16)) == 0


def test_argument_errors_of_all_four_entries():
    """every refusal comes back before anything is launched or written: the device entries are called here with HOST
    pointers, which they never dereference on these paths"""
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import lib, ptr
    N, ev, _ = R.wide_case()
    tc, _keep = _tcsr(W.library_graph(N, ev))
    T = 16
    among = np.arange(1, 41, dtype=np.int64)
    ids, counts = np.full(T, -7, np.int64), np.full(T, -7, np.int32)
    nv, nd = np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    ws = np.zeros(1 << 15, np.uint8)
    nan = float('nan')

    def trend(entry, g=C.byref(tc), lo=0.0, hi=10.0, am=ptr(among), M=40, Tt=T, o_ids=ptr(ids), o_counts=ptr(counts), o_nv=ptr(nv),
              o_nd=ptr(nd), w=ptr(ws), wb=ws.nbytes):
        args = (g, lo, hi, am, M, Tt, o_ids, o_counts, o_nv, o_nd)
        return entry(*args) if entry is lib.tg_trending_host else entry(*args, w, wb, None)

    bad = [dict(Tt=0), dict(Tt=R.TREND_MAX + 1), dict(M=-1), dict(lo=11.0), dict(lo=nan), dict(hi=nan), dict(lo=nan, hi=nan), dict(g=None),
           dict(o_ids=None), dict(o_counts=None), dict(o_nv=None), dict(o_nd=None)]
    for entry in (lib.tg_trending_host, lib.tg_trending):
        for kw in bad:
            assert trend(entry, **kw) == _lib.TG_EINVAL, (entry.__name__, kw)
    need = int(lib.tg_trending_workspace_bytes(40, T))
    assert trend(lib.tg_trending, wb=need - 1) == _lib.TG_EWORKSPACE and trend(lib.tg_trending, w=None) == _lib.TG_EWORKSPACE
    assert (ids == -7).all() and (counts == -7).all() and (nv == -7).all() and (nd == -7).all()
    assert trend(lib.tg_trending_host) == _lib.TG_OK and trend(lib.tg_trending_host, am=None, M=0) == _lib.TG_OK
    assert trend(lib.tg_trending_host, lo=10.0) == _lib.TG_OK and nv[0] == 0              # t_lo == t_hi: an empty window
    # M == 0: all zeros; ids outside the graph have no entries (the Python front refuses them)
    assert trend(lib.tg_trending_host, M=0) == _lib.TG_OK and not ids.any() and not counts.any() and nv[0] == 0 and nd[0] == 0
    out = np.array([-1, N, 9, 1 << 40], np.int64)
    assert trend(lib.tg_trending_host, am=ptr(out), M=4, hi=1e9) == _lib.TG_OK and ids[:2].tolist() == [9, 0] and nd[0] == 1

    B, Cn = 3, 8
    src, ts = np.array([1, 2, 3], np.int64), np.full(3, 50.0)
    r_ids, r_counts = np.full((B, Cn), -7, np.int64), np.full((B, Cn), -7, np.int32)
    r_nv, r_nf = np.zeros(B, np.int32), np.full(B, -7, np.int32)
    fill_ids, n_fill = np.arange(1, T + 1, dtype=np.int64), np.array([T], np.int32)

    def fill(entry, g=C.byref(tc), Bq=B, s=ptr(src), t=ptr(ts), Cc=Cn, o_ids=ptr(r_ids), o_counts=ptr(r_counts), o_nv=ptr(r_nv),
             f=ptr(fill_ids), nf=ptr(n_fill), Tt=T, flags=0, o_nf=ptr(r_nf)):
        args = (g, Bq, s, t, Cc, o_ids, o_counts, o_nv, f, nf, Tt, flags, o_nf)
        return entry(*args) if entry is lib.tg_fill_candidates_host else entry(*args, None)

    bad = [dict(Bq=-1), dict(g=None), dict(s=None), dict(t=None), dict(o_ids=None), dict(o_counts=None), dict(o_nv=None), dict(f=None),
           dict(nf=None), dict(o_nf=None), dict(Cc=0), dict(Cc=W.MAX_ENDPOINTS + 1), dict(Tt=0), dict(Tt=R.TREND_MAX + 1), dict(flags=4),
           dict(flags=-1)]
    for entry in (lib.tg_fill_candidates_host, lib.tg_fill_candidates):
        for kw in bad:
            assert fill(entry, **kw) == _lib.TG_EINVAL, (entry.__name__, kw)
        assert fill(entry, Bq=0, s=None, t=None, o_ids=None, o_counts=None, o_nv=None, f=None, nf=None, o_nf=None) == _lib.TG_OK
    assert (r_ids == -7).all() and (r_counts == -7).all() and not r_nv.any() and (r_nf == -7).all()
    # a source outside the graph is a node without entries (the Python front refuses it)
    assert fill(lib.tg_fill_candidates_host, s=ptr(np.array([1, N, -1], np.int64)), flags=1) == _lib.TG_OK
    assert r_nf.tolist()[1:] == [Cn, Cn] and r_ids[1].tolist() == list(range(1, Cn + 1))


def test_python_fronts_refuse_by_name():
    from www2023tiger_amd import hip_ops
    N, ev, _ = R.wide_case()
    g = W.library_graph(N, ev)
    for T in (0, R.TREND_MAX + 1):
        with pytest.raises(ValueError, match='TG_TREND_MAX'):
            hip_ops.trending(g, 10.0, T)
    for window in (0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='window'):
            hip_ops.trending(g, 10.0, 16, window=window)
    with pytest.raises(ValueError, match='NaN'):
        hip_ops.trending(g, float('nan'), 16)
    with pytest.raises(ValueError, match='among.*duplicate'):
        hip_ops.trending(g, 10.0, 16, among=torch.tensor([3, 4, 3]))
    for bad in ([3, N], [-1, 3]):
        with pytest.raises(ValueError, match='among.*outside'):
            hip_ops.trending(g, 10.0, 16, among=torch.tensor(bad))
    out = hip_ops.trending(g, 10.0, 16, among=torch.zeros(0, dtype=torch.int64))
    assert not out['ids'].any() and out['n_valid'].tolist() == [0] and out['n_distinct'].tolist() == [0]

    s, t = torch.tensor([1, 2, 3]), torch.full((3,), 50.0, dtype=torch.float64)
    cand = hip_ops.walk_candidates(g, s, t, 8)
    trend = hip_ops.trending(g, 50.0, 16)
    with pytest.raises(ValueError, match='source id'):
        hip_ops.fill_candidates(g, torch.tensor([1, N, 2]), t, cand, trend)
    with pytest.raises(ValueError, match='3 sources'):
        hip_ops.fill_candidates(g, s, t[:2], cand, trend)
    with pytest.raises(ValueError, match='3 sources'):
        hip_ops.fill_candidates(g, s, t, dict(cand, n_valid=cand['n_valid'][:2]), trend)
    with pytest.raises(ValueError, match="'counts'"):
        hip_ops.fill_candidates(g, s, t, dict(ids=cand['ids'], n_valid=cand['n_valid']), trend)
    with pytest.raises(ValueError, match='trend'):
        hip_ops.fill_candidates(g, s, t, cand, dict(ids=trend['ids']))
    with pytest.raises(ValueError, match='int64'):
        hip_ops.fill_candidates(g, s, t, dict(cand, ids=cand['ids'].int()), trend)
    with pytest.raises(ValueError, match='TG_TREND_MAX'):
        hip_ops.fill_candidates(g, s, t, cand, dict(ids=torch.zeros(R.TREND_MAX + 1, dtype=torch.int64), n_valid=trend['n_valid']))
    with pytest.raises(ValueError, match='TG_TREND_MAX'):
        hip_ops.fill_candidates(g, s, t, cand, dict(ids=torch.zeros(0, dtype=torch.int64), n_valid=trend['n_valid']))
    out = hip_ops.fill_candidates(g, s, t, cand, trend, exclude_seen=True)
    assert out['n_distinct'] is cand['n_distinct'] and torch.equal(out['n_valid'], cand['n_valid'] + out['n_filled'])
    none = hip_ops.fill_candidates(g, s[:0], t[:0], {k: v[:0] for k, v in cand.items()}, trend)
    assert none['ids'].shape == (0, 8) and none['n_filled'].shape == (0,) and none['n_filled'].dtype == torch.int32


def test_signatures():
    import inspect
    from www2023tiger_amd import eval_utils, hip_ops
    from www2023tiger_amd.model.tiger import TIGE
    q = inspect.signature(TIGE.recommend_walk).parameters
    assert q['fill'].default is None and q['fill'].kind is inspect.Parameter.KEYWORD_ONLY
    assert q['C'].default == 256 and q['chunk_queries'].default == 65536 and q['uptodate'].default is None
    assert list(inspect.signature(eval_utils.eval_recommendation).parameters)[-1] == 'catalogue_at'
    p = inspect.signature(hip_ops.trending).parameters
    assert list(p)[:3] == ['graph', 't', 'T'] and p['window'].default is None and p['among'].default is None
    f = inspect.signature(hip_ops.fill_candidates).parameters
    assert list(f)[:5] == ['graph', 'src', 'ts', 'cand', 'trend'] and f['exclude_seen'].default is False and f['keep_self'].default is False
    with pytest.raises(ValueError, match='fill'):
        eval_utils.eval_recommendation(None, None, 'cpu', walk=dict(C=16, fill=dict(window=3.0)))
    with pytest.raises(ValueError, match='TG_TREND_MAX'):
        eval_utils.eval_recommendation(None, None, 'cpu', walk=dict(C=16, fill=dict(T=R.TREND_MAX + 1)))
    with pytest.raises(ValueError, match='window'):
        eval_utils.eval_recommendation(None, None, 'cpu', walk=dict(C=16, fill=dict(T=16, window=-1.0)))
