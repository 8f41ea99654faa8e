"""Late events on the GPU: tg_tcsr_merge / Graph.merged against the host twin (itself held against numpy and the host builder in
tests/test_tcsr_merge_host.py), all four arrays bit for bit, at the sizes where the kernels change path: around the
one-workgroup sort's cap, around the copy tile, more cut points inside one tile than its staged window holds, keys that differ
in one radix word only.  Nothing is written outside the out arrays or into the parent; the samplers on a merged graph against
the same calls on a graph built from scratch."""
import ctypes as C

import numpy as np
import pytest
import torch

from _merge_ref import CASES, as_batch, assert_same, concat, host_build, host_merge, late_batch, random_tcsr, stream

pytestmark = pytest.mark.gpu

MG_SMALL, AP_TILE, AP_WIN = 4096, 2048, 4096   # tg_append.hip: one-workgroup sort, old entries per copy block, staged cuts
GUARD = 0x5A
NAMES = ('indptr', 'ts', 'nbr', 'eid')


def dev():
    return torch.device('cuda', 0)


def raw_merge(h, N, new, *, ws_bytes=None):
    """tg_tcsr_merge over uploaded host arrays h, into out arrays with 64 guard bytes behind each -> (rc, outs, sizes, need)"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    d = dev()
    g_dev = [torch.from_numpy(a).to(d) for a in h]
    N0, P0, n = len(h[0]) - 1, len(h[1]), len(new[0])
    P = P0 + 2 * n
    sizes = [(N + 1) * 8, P * 8, P * 4, P * 4]
    outs = [torch.full((sz + 64,), GUARD, dtype=torch.uint8, device=d) for sz in sizes]
    batch = [torch.from_numpy(a).to(d) for a in new]
    need = int(lib.tg_tcsr_merge_workspace_bytes(P0, n, N0, N))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=d)
    g = TgTcsr(N0, P0, *(ptr(x) for x in g_dev))
    rc = lib.tg_tcsr_merge(C.byref(g), N, n, *(ptr(b) for b in batch), *(ptr(o) for o in outs), ptr(ws), nbytes, stream_ptr(d))
    torch.cuda.synchronize()
    for a, b, nm in zip(g_dev, h, NAMES):
        np.testing.assert_array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8), err_msg=f'the parent\'s {nm} was written')
    return rc, outs, sizes, need


def check_raw(h, N, new, what):
    rc, outs, sizes, _ = raw_merge(h, N, new)
    assert rc == 0, what
    rc, want = host_merge(h, N, new)
    assert rc == 0
    for o, sz, w, nm in zip(outs, sizes, want, NAMES):
        assert bool((o[sz:] == GUARD).all()), f'{what} {nm}: bytes behind the array were written'
        np.testing.assert_array_equal(o[:sz].cpu().numpy(), w.view(np.uint8), err_msg=f'{what} {nm}')


@pytest.mark.parametrize('case', list(CASES))
def test_device_merge_equals_the_host_twin_on_the_host_cases(case):
    N0, N, old, new = CASES[case]
    check_raw(host_build(N0, *old), N, new, case)


# new entries m = 2 n around the one-workgroup cap, and the smallest batches
@pytest.mark.parametrize('n', [1, 2, MG_SMALL // 2 - 1, MG_SMALL // 2, MG_SMALL // 2 + 1])
def test_batch_sizes_around_the_one_workgroup_sort(n):
    N = 400
    h = random_tcsr(N, 3001, seed=n)
    check_raw(h, N, late_batch(N, n, n + 1, -4, 3001 / 6.0 + 4), f'n={n}')


# old entry counts around the copy tile - odd counts belong to no event list: the row-wise definition
@pytest.mark.parametrize('P0', [0, 1, AP_TILE - 1, AP_TILE, AP_TILE + 1, 2 * AP_TILE + 1])
def test_old_entry_counts_around_the_copy_tile(P0):
    N = 37
    h = random_tcsr(N, P0, seed=P0 + 5)
    check_raw(h, N, late_batch(N, 150, P0 + 6, -2, max(P0 / 6.0, 4.0) + 2), f'P0={P0}, small path')
    check_raw(h, N + 3, late_batch(N + 3, MG_SMALL // 2 + 7, P0 + 7, -2, max(P0 / 6.0, 4.0) + 2), f'P0={P0}, large path, growth')


def test_more_cut_points_inside_one_tile_than_the_staged_window_holds():
    """a hub row of about 3 000 old entries takes about 5 000 late entries with times spread through the half of it that
    lies in the first 2 048-entry tile: that tile holds more than AP_WIN cut points strictly inside it and searches them in
    global memory (the count is worked out here, from the arrays, before anything runs)"""
    N = 20
    h = random_tcsr(N, 3300, seed=31, t_hi=3000.0, rows=[7] * 10 + [3])
    assert h[0][8] - h[0][7] > 2800
    new = late_batch(N, 2700, 32, 100.0, 1500.0, hub=7, floor=False)
    j = np.arange(2 * len(new[0]))
    owner = np.where(j & 1, new[1][j >> 1], new[0][j >> 1])
    t7 = np.sort(new[2][j[owner == 7] >> 1])
    cuts = h[0][7] + np.searchsorted(h[1][h[0][7]:h[0][8]], t7, side='right')
    inside = max(int(((cuts > p0) & (cuts <= min(p0 + AP_TILE, len(h[1])) - 1)).sum()) for p0 in range(0, len(h[1]), AP_TILE))
    assert inside > AP_WIN, inside
    check_raw(h, N, new, 'unstaged window')


def test_keys_that_differ_in_one_radix_word_only_and_negative_times():
    N, n = 90, MG_SMALL // 2 + 300   # the large path: three radix sorts
    h = random_tcsr(N, 2500, seed=41, t_hi=8.0)
    rs = np.random.RandomState(42)
    base = late_batch(N, n, 43, 0, 1)
    lo_only = (np.float64(3.0).view(np.uint64) + rs.randint(0, 2 ** 32, n).astype(np.uint64)).view(np.float64)   # in [3, 3 + 2^-20)
    hi_only = ((rs.randint(0x3FF00000, 0x40200000, n).astype(np.uint64) << np.uint64(32)) | np.uint64(0x12345678)).view(np.float64)
    assert len(np.unique(lo_only.view(np.uint64) >> np.uint64(32))) == 1
    assert len(np.unique(hi_only.view(np.uint64) & np.uint64(0xFFFFFFFF))) == 1 and hi_only.min() >= 1.0 and hi_only.max() < 8.0
    neg = -np.abs(rs.standard_cauchy(n)) * 3 + 2.0   # mostly negative, a few positive: the key flips at the sign
    neg[::50] = -0.0
    for ts, what in ((lo_only, 'low word only'), (hi_only, 'high word only'), (neg, 'negative times')):
        check_raw(h, N, as_batch((base[0], base[1], ts, base[3])), what)
    hn = random_tcsr(N, 2500, seed=44, t_hi=40.0)
    hn = (hn[0], np.ascontiguousarray(hn[1] - 20.0), hn[2], hn[3])   # negative times in the old rows too
    check_raw(hn, N, as_batch((base[0], base[1], np.floor(neg), base[3])), 'negative times on both sides')
    check_raw(hn, N, tuple(a[:200] for a in as_batch((base[0], base[1], np.floor(neg), base[3]))), 'the same, one workgroup')


@pytest.mark.parametrize('n', [200, MG_SMALL // 2 + 50])
def test_a_short_workspace_is_refused_before_any_launch(n):
    from www2023tiger_amd import _lib
    N = 60
    h = random_tcsr(N, 700, seed=51)
    new = late_batch(N, n, 52, 0, 120)
    need = raw_merge(h, N, new)[3]
    assert need > 0
    for short in (0, need // 2, need - 256 - 16):
        rc, outs, _, _ = raw_merge(h, N, new, ws_bytes=short)
        assert rc == _lib.TG_EWORKSPACE
        assert all(bool((o == GUARD).all()) for o in outs), 'something was launched'


# ------------------------------------------------------------------------------------------------------- Graph.merged
def graph_of(N, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    kw.setdefault('device', dev())
    return Graph.from_arrays(*ev, max_node_id=N - 1, **kw)


def arrays(g):
    return [t.cpu().numpy() for t in g._tensors()]


@pytest.mark.parametrize('case', ['inside', 'hub', 'growth', 'n0'])
def test_merged_on_a_device_resident_parent(case):
    from www2023tiger_amd import hip_ops
    N0, N, old, new = CASES[case]
    g0 = graph_of(N0, old, strategy='recent_nodes', seed=4)
    before = arrays(g0)
    assert g0._dev is not None
    g1 = g0.merged(*new, num_node=None if N == N0 else N)
    assert g1._dev is not None and g1._log is None and g1._root is not g0._root and g1.num_node == N
    want = host_build(N, *concat(old, new))
    assert_same(arrays(g1), want, case)
    assert_same(arrays(g0), before, 'the parent is unchanged')
    assert g1.tcsr.num_entry == len(want[1]) and g1.tcsr.serial == g1.serial != g0.serial
    assert hip_ops.tcsr_verify(g1)[0] == 0
    assert_same(g1._host_tcsr(), want, case + ' (host view, downloaded)')
    assert g1._events is None and g1._time_ordered == (len(new[0]) == 0) and g1._mt is g0._mt and g1.rng is g0.rng
    t_all = np.concatenate([old[2], new[2]])
    assert float(g1._t_last) == t_all.max()


def test_device_tensor_inputs_checked_and_trusted_and_what_is_refused():
    N0, N, old, new = CASES['inside']
    g0 = graph_of(N0, old)
    before = arrays(g0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    want = host_build(N, *concat(old, new))
    for validate in (True, False):
        g1 = g0.merged(*(t(a) for a in new), validate=validate)
        assert_same(arrays(g1), want, f'validate={validate}')
        assert float(g1._t_last) == max(old[2].max(), new[2].max())
    assert torch.is_tensor(g1._t_last)   # trusted: the latest time stayed on the device
    # a later on-time batch after a trusted merge: `extended` resolves the device-side latest time
    late_t = float(g1._t_last)
    g2 = g1.extended(np.array([1]), np.array([2]), np.array([late_t]), np.array([5]))
    assert g2.tcsr.num_entry == g1.tcsr.num_entry + 2

    def bad(col, idx, val):
        b = [a.copy() for a in new]
        b[col][idx] = val
        return [t(a) for a in b]
    for col, idx, val, msg in ((2, 40, np.nan, 'NaN'), (0, 3, N0, 'node ids'), (1, 3, -1, 'node ids'), (3, 3, 2 ** 31, '31 bits'),
                               (3, 3, -1, '31 bits')):
        with pytest.raises(ValueError, match=msg):
            g0.merged(*bad(col, idx, val))
    with pytest.raises(ValueError, match='no row of the edge table'):
        g0.merged(*bad(3, 3, 77), eid_rows=77)
    with pytest.raises(ValueError, match='auto'):
        g0.merged(*(t(a) for a in new), validate=False, num_node='auto')
    assert_same(arrays(g0), before, 'nothing ran')


@pytest.mark.parametrize('strategy', ['recent_edges', 'recent_nodes', 'uniform'])
def test_samplers_and_history_on_a_merged_graph_equal_a_graph_from_scratch(strategy):
    N = 300
    s = stream(N, 2600, seed=61, hub=7)
    late = np.random.RandomState(62).uniform(size=2600) < 0.3
    late[:200] = False
    on_time, held = as_batch(tuple(a[~late] for a in s)), as_batch(tuple(a[late] for a in s))
    perm = np.random.RandomState(63).permutation(len(held[0]))
    held = tuple(np.ascontiguousarray(a[perm]) for a in held)
    full = concat(on_time, held)   # what from_arrays sorts stably per node: the same rows
    g = graph_of(N, on_time, strategy=strategy, seed=5)
    g._tensors()
    g = g.merged(*held)
    ref = graph_of(N, full, strategy=strategy, seed=5)
    rs = np.random.RandomState(3)
    q = torch.from_numpy(np.concatenate([rs.randint(0, N, 500), s[0][-200:], s[1][-200:]])).to(dev())
    qt = torch.from_numpy(np.concatenate([rs.uniform(0, s[2][-1] + 2, 500), s[2][-200:], s[2][-200:] + 1])).to(dev())
    for K in (1, 10):
        for _ in range(2):   # 'uniform': the second call continues the stream where the first left it, on both
            got, want = g.sample_device(q, qt, K), ref.sample_device(q, qt, K)
            for a, b, nm in zip(got, want, ('nbr', 'eid', 'ts', 'dir')):
                assert torch.equal(a, b), f'{strategy} K={K} {nm}'
    assert bool((got[0] != 0).any())
    qn, qtn = q.cpu().numpy(), qt.cpu().numpy()
    for a, b in zip(g.get_history(qn, qtn, 7), ref.get_history(qn, qtn, 7)):
        np.testing.assert_array_equal(a, b)
