"""T-CSR erase on the GPU: tg_tcsr_erase_plan + tg_tcsr_erase_apply / Graph.without on a device-resident parent against the
host twin (which tests/test_tcsr_erase_host.py holds against numpy and against the build over the filtered events), all
four arrays bit for bit, at the shapes where the kernels can go wrong: entry counts at the seams of the 2048-entry tile,
node counts at the seams of the 256-slot chunks, a hub row over three tiles, a tile whose owner window exceeds the LDS
window, a tile that loses everything beside one that keeps everything, either bitmap NULL, an eid bitmap shorter than the
eids; nothing written outside the out arrays; the same result on a second stream; the samplers, the walk and the trending
list on an erased graph against a graph built from scratch.

Synthetic T-CSR arrays (`synth`) carry what no event stream gives - odd entry counts, a single node - and need not be the
T-CSR of a stream: neither the device path nor the host twin looks at anything but row bounds, neighbours and eids.

The kernels launch one workgroup per tile / chunk (tg_erase.hip: `n_tile`, `cdiv(n_tile + 1, ES_THREADS)`,
`cdiv(num_node + 1, ES_THREADS)`): no grid is capped, so there is no size past a cap to test."""
import ctypes as C

import numpy as np
import pytest
import torch

from _append_ref import NAMES, assert_same, host_build, stream
from _erase_ref import bitmap, erase_by_build, erase_numpy, filtered, host_erase, small_eids
from _trim_ref import events

pytestmark = pytest.mark.gpu

ES_TILE, ES_CHUNK, ES_WIN = 2048, 256, 2048   # tg_erase.hip: ES_TILE, ES_THREADS (slots per chunk), ES_WIN
GUARD = 0x5A


def dev():
    return torch.device('cuda', 0)


def synth(N, P, seed=0, deg=None):
    """host T-CSR arrays of N rows and P entries: random row lengths (or `deg`), times ascending inside a row, random
    neighbours, eids in [0, 4 P] with a random bit 31"""
    rs = np.random.RandomState(seed)
    if deg is None:
        deg = np.bincount(rs.randint(0, N, P), minlength=N)
    deg = np.asarray(deg, dtype=np.int64)
    assert len(deg) == N and deg.sum() == P
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    owner = np.repeat(np.arange(N), deg)
    ts = np.floor(rs.uniform(0, 50, P))
    ts = ts[np.lexsort((ts, owner))] if P else ts
    nbr = rs.randint(0, N, P).astype(np.int32)
    eid = (rs.randint(0, 4 * P + 1, P).astype(np.uint32) | (rs.randint(0, 2, P).astype(np.uint32) << np.uint32(31))).view(np.int32)
    return indptr, ts.astype(np.float64), nbr, eid


def raw_erase(h, S=None, R=None, n_rows=None, *, ws_bytes=None, stream=None):
    """plan + read-back + apply on the device into out arrays with 64 guard bytes behind each -> (rc of plan, rc of apply,
    outs, sizes).  S / R: ids or None (a NULL bitmap)"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    d = dev()
    N, P = len(h[0]) - 1, len(h[1])
    if R is not None and n_rows is None:
        n_rows = int(np.max(R)) + 1 if len(R) else 0
    n_rows = 0 if n_rows is None else int(n_rows)
    g_dev = [torch.from_numpy(a).to(d) for a in h]
    nb = None if S is None else torch.from_numpy(bitmap(S, N)).to(d)
    eb = None if R is None else torch.from_numpy(np.concatenate([bitmap(R, n_rows), np.zeros(1, dtype=np.int64)])).to(d)
    need = int(lib.tg_tcsr_erase_workspace_bytes(N, P))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.full((need,), GUARD, dtype=torch.uint8, device=d)
    g = TgTcsr(N, P, *(ptr(x) for x in g_dev))
    indptr = torch.full(((N + 1) * 8 + 64,), GUARD, dtype=torch.uint8, device=d)
    st = stream_ptr(d) if stream is None else stream.cuda_stream
    torch.cuda.synchronize()
    rc_plan = lib.tg_tcsr_erase_plan(C.byref(g), ptr(nb), ptr(eb), n_rows, ptr(indptr), ptr(ws), nbytes, st)
    torch.cuda.synchronize()
    if rc_plan != 0:
        return rc_plan, None, [indptr, ws], need
    K = int(indptr[:(N + 1) * 8].view(torch.int64)[-1])
    assert 0 <= K <= P
    sizes = [(N + 1) * 8, K * 8, K * 4, K * 4]
    outs = [indptr] + [torch.full((sz + 64,), GUARD, dtype=torch.uint8, device=d) for sz in sizes[1:]]
    torch.cuda.synchronize()   # (the guard fills run on the current stream, the apply maybe on another)
    rc_apply = lib.tg_tcsr_erase_apply(C.byref(g), ptr(indptr), K, *(ptr(o) for o in outs[1:]), ptr(ws), nbytes, st)
    torch.cuda.synchronize()
    return rc_plan, rc_apply, outs, sizes


def check_raw(h, S=None, R=None, n_rows=None, what='', **kw):
    rc_plan, rc_apply, outs, sizes = raw_erase(h, S, R, n_rows, **kw)
    assert rc_plan == 0 and rc_apply == 0, what
    rc, want, kept = host_erase(h, S, R, n_rows)
    assert rc == 0 and sizes[1] == 8 * kept, f'{what}: {sizes[1] // 8} kept entries on the device, {kept} on the host'
    for o, sz, w, nm in zip(outs, sizes, want, NAMES):
        assert bool((o[sz:] == GUARD).all()), f'{what} {nm}: bytes behind the array were written'
        np.testing.assert_array_equal(o[:sz].cpu().numpy(), np.ascontiguousarray(w).view(np.uint8), err_msg=f'{what} {nm}')
    return want, kept


def marks(N, P, seed):
    """a fifth of the nodes and a fifth of the eid range"""
    rs = np.random.RandomState(seed)
    S = rs.choice(N, size=max(1, N // 5), replace=False)
    R = rs.choice(4 * P + 1, size=max(1, (4 * P + 1) // 5), replace=False)
    return S.astype(np.int64), R.astype(np.int64)


@pytest.mark.parametrize('P', [0, 1, ES_TILE - 1, ES_TILE, ES_TILE + 1, 2 * ES_TILE + 1])
def test_entry_counts_at_the_tile_seams_and_node_counts_at_the_chunk_seams(P):
    for N in (1, ES_CHUNK - 1, ES_CHUNK, ES_CHUNK + 1):
        h = synth(N, P, seed=N + P)
        S, R = marks(N, P, seed=N)
        for what, s, r in (('S', S, None), ('R', None, R), ('both', S, R)):
            _, kept = check_raw(h, s, r, what=f'N={N} P={P} {what}')
            if P > 1 and not (N == 1 and what == 'S' and 0 not in S):
                assert kept < P, 'nothing was dropped: the case checks nothing'
        assert check_raw(h, None, None, what='both NULL')[1] == P
        assert check_raw(h, [], [], what='nothing marked')[1] == P


def test_a_hub_row_over_three_tiles_partly_erased_through_its_neighbours():
    N, hub = 300, 7
    deg = np.full(N, 3, dtype=np.int64)
    deg[hub] = 5000
    h = synth(N, int(deg.sum()), seed=5, deg=deg)
    b, e = int(h[0][hub]), int(h[0][hub + 1])
    assert e - b == 5000 and (e - 1) // ES_TILE - b // ES_TILE >= 2
    S = np.arange(20, 120)   # neighbours of the hub, not the hub
    want, kept = check_raw(h, S, None, what='hub')
    row = np.diff(want[0])[hub]
    assert ES_TILE < row < 5000   # partly erased, still more than a tile
    check_raw(h, [hub], None, what='the hub itself')
    check_raw(h, S, np.arange(0, 4 * len(h[1]), 3), what='hub, S and R')


def test_a_tile_over_thousands_of_empty_rows_searches_global_memory():
    N = 6000
    deg = np.zeros(N, dtype=np.int64)
    deg[1], deg[2 + ES_WIN + 500], deg[N - 1] = 30, 40, 25   # more than ES_WIN consecutive empty rows inside one tile
    h = synth(N, int(deg.sum()), seed=6, deg=deg)
    owner = lambda p: int(np.searchsorted(h[0], p, 'right')) - 1
    assert owner(len(h[1]) - 1) - owner(0) > ES_WIN and len(h[1]) < ES_TILE
    rs = np.random.RandomState(1)
    S = np.concatenate([rs.choice(N, 1500, replace=False), [2 + ES_WIN + 500]])
    S = S[S != 1]   # (row 1 stays and loses the entries whose neighbour goes)
    want, kept = check_raw(h, S, None, what='sparse')
    assert 0 < kept < len(h[1]) and np.diff(want[0])[2 + ES_WIN + 500] == 0
    check_raw(h, [1], np.arange(50), what='sparse, S and R')
    # two tiles: the first inside a few dense rows (its window is staged), the second over the sparse tail
    deg[:8] = 300
    h = synth(N, int(deg.sum()), seed=7, deg=deg)
    assert ES_TILE < len(h[1]) <= 2 * ES_TILE and owner(ES_TILE - 1) - owner(0) <= ES_WIN < owner(len(h[1]) - 1) - owner(ES_TILE)
    check_raw(h, S, None, what='dense then sparse')


def test_a_tile_that_loses_everything_beside_a_tile_that_keeps_everything():
    deg = np.array([ES_TILE, ES_TILE, ES_TILE], dtype=np.int64)
    indptr, ts, nbr, eid = synth(3, 3 * ES_TILE, seed=8, deg=deg)
    nbr = np.repeat(np.array([0, 1, 0], dtype=np.int32), ES_TILE)   # rows 0 and 2 talk to node 0, row 1 to itself
    h = (indptr, ts, nbr, eid)
    want, kept = check_raw(h, [1], None, what='the middle tile goes')
    assert kept == 2 * ES_TILE and np.diff(want[0]).tolist() == [ES_TILE, 0, ES_TILE]
    want, kept = check_raw(h, [0], None, what='the outer tiles go')
    assert kept == ES_TILE and np.diff(want[0]).tolist() == [0, ES_TILE, 0]
    eid = np.arange(3 * ES_TILE, dtype=np.int32)   # by eid: the first tile goes, the others stay
    want, kept = check_raw((indptr, ts, nbr, eid), None, np.arange(ES_TILE), what='the first tile goes')
    assert kept == 2 * ES_TILE and np.diff(want[0]).tolist() == [0, ES_TILE, ES_TILE]


def test_null_bitmaps_and_an_eid_bitmap_shorter_than_the_eids():
    N, P = 500, 5000
    h = synth(N, P, seed=9)
    S, R = marks(N, P, seed=9)
    assert check_raw(h, S, None, what='eid_bits NULL')[1] < P
    assert check_raw(h, None, R, what='node_bits NULL')[1] < P
    assert check_raw(h, None, None, what='both NULL')[1] == P
    big = int((h[3].view(np.uint32) & 0x7FFFFFFF).max())
    n_rows = big // 2
    assert (R >= n_rows).any() and (R < n_rows).any()
    _, kept_short = check_raw(h, None, R, n_rows, what='n_rows below the largest eid')
    assert kept_short > check_raw(h, None, R, what='R')[1]
    assert check_raw(h, None, R, 0, what='n_rows = 0')[1] == P


def test_a_short_workspace_is_refused_before_any_launch():
    from www2023tiger_amd import _lib
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    N, P = 1000, 4096
    h = synth(N, P, seed=10)
    S, R = marks(N, P, seed=10)
    need = int(lib.tg_tcsr_erase_workspace_bytes(N, P))
    assert need >= P // 8
    for short in (0, need // 2, need - 1):
        rc, _, (indptr, ws), _ = raw_erase(h, S, R, ws_bytes=short)
        assert rc == _lib.TG_EWORKSPACE
        assert bool((indptr == GUARD).all()) and bool((ws == GUARD).all()), 'something was launched'
    rc, _, (indptr, ws), _ = raw_erase(h, S, R, n_rows=-1)
    assert rc == _lib.TG_EINVAL and bool((indptr == GUARD).all()) and bool((ws == GUARD).all())
    # apply: a short workspace, and an entry count that no erase of this graph can have
    rc_plan, rc_apply, outs, sizes = raw_erase(h, S, R)
    assert rc_plan == 0 and rc_apply == 0
    g_dev = [torch.from_numpy(a).to(dev()) for a in h]
    g = TgTcsr(N, P, *(ptr(x) for x in g_dev))
    fresh = [torch.full((sz + 64,), GUARD, dtype=torch.uint8, device=dev()) for sz in sizes[1:]]
    ws = torch.zeros(need, dtype=torch.uint8, device=dev())
    K = sizes[1] // 8
    assert lib.tg_tcsr_erase_apply(C.byref(g), ptr(outs[0]), K, *(ptr(o) for o in fresh), ptr(ws), need - 1,
                                   stream_ptr(dev())) == _lib.TG_EWORKSPACE
    for bad in (-1, P + 1):
        assert lib.tg_tcsr_erase_apply(C.byref(g), ptr(outs[0]), bad, *(ptr(o) for o in fresh), ptr(ws), need,
                                       stream_ptr(dev())) == _lib.TG_EINVAL
    assert lib.tg_tcsr_erase_apply(C.byref(g), ptr(outs[0]), 0, None, None, None, ptr(ws), need, stream_ptr(dev())) == 0
    torch.cuda.synchronize()
    assert all(bool((o == GUARD).all()) for o in fresh), 'something was launched'


def test_a_second_stream_gives_the_same_four_arrays():
    N, P = 700, 3 * ES_TILE + 77
    h = synth(N, P, seed=11)
    S, R = marks(N, P, seed=11)
    a = raw_erase(h, S, R)
    side = torch.cuda.Stream(device=dev())
    b = raw_erase(h, S, R, stream=side)
    assert a[:2] == (0, 0) and b[:2] == (0, 0) and a[3] == b[3]
    for x, y, nm in zip(a[2], b[2], NAMES):
        assert torch.equal(x, y), nm
    check_raw(h, S, R, what='second stream', stream=side)


# ----------------------------------------------------------------------------------------------- Graph.without, resident
def graph_of(N, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    kw.setdefault('device', dev())
    return Graph.from_arrays(*ev, max_node_id=N - 1, **kw)


def arrays(g):
    return [t.cpu().numpy() for t in g._tensors()]


def resident(N, ev, **kw):
    g = graph_of(N, ev, **kw)
    g._tensors()
    assert g._dev is not None
    return g


def picks(N, ev, seed=0):
    rs = np.random.RandomState(seed)
    ids = np.unique(np.concatenate([ev[0], ev[1]]))
    ids = ids[ids != 0]
    S = rs.choice(ids, size=max(1, len(ids) // 5), replace=False)
    R = rs.choice(ev[3], size=max(1, len(ev[3]) // 4), replace=False)
    return S.astype(np.int64), R.astype(np.int64)


@pytest.mark.parametrize('name,N,E,hub', [('N65', 65, 201, None), ('N1000', 1000, 2048, None), ('hub', 300, 4000, 7)])
def test_without_on_the_device_equals_the_host_twin_and_the_build_over_the_filtered_events(name, N, E, hub):
    ev = small_eids(events(stream(N, E, seed=3, hub=hub)))
    g0 = resident(N, ev, strategy='recent_edges', seed=3)
    before = arrays(g0)
    h = host_build(N, *ev)
    assert_same(before, h, 'the parent')
    S, R = picks(N, ev, seed=1)
    if hub is not None:
        S = S[S != hub]
    for what, s, r in (('S', S, None), ('R', None, R), ('both', torch.as_tensor(S).to(dev()), torch.as_tensor(R)),
                       ('none', [], []), ('all', np.arange(1, N), ev[3]), ('absent', None, [10 ** 6])):
        g1 = g0.without(nodes=s, eids=r)
        s_np = None if s is None else np.asarray(s.cpu() if torch.is_tensor(s) else s, dtype=np.int64)
        r_np = None if r is None else np.asarray(r.cpu() if torch.is_tensor(r) else r, dtype=np.int64)
        want = erase_numpy(h, s_np, r_np)
        got = arrays(g1)
        assert_same(got, want, f'{name} {what}')
        assert_same(got, erase_by_build(N, ev, s_np, r_np), f'{name} {what} (build over the filtered events)')
        kept = len(want[1])
        assert g1.tcsr.num_entry == kept == g1._dev[1].numel() and g1.tcsr.serial == g1.serial != g0.serial
        assert g1._dev[1].untyped_storage().nbytes() == 8 * kept   # allocated exactly
        assert g1._events is None and g1._t_last == g0._t_last and g1._mt is g0._mt and g1.rng is g0.rng
        assert (g1.strategy, g1.seed, g1._time_ordered, g1.num_node) == (g0.strategy, g0.seed, g0._time_ordered, N)
        assert_same(g1._host_tcsr(), want, f'{name} {what} (host view)')
        if what == 'all':
            assert kept == 0
            g2 = g1.extended(ev[0][:5], ev[1][:5], ev[2][-1:].repeat(5), np.arange(5000, 5005))   # `extended` still works
            assert g2.tcsr.num_entry == 10
    assert_same(arrays(g0), before, 'the parent is unchanged')
    with pytest.raises(ValueError, match='padding id'):
        g0.without(nodes=torch.tensor([4, 0], device=dev()))
    with pytest.raises(ValueError, match=r'\[0, num_node\)'):
        g0.without(nodes=[N])
    with pytest.raises(ValueError, match='non-negative'):
        g0.without(eids=torch.tensor([-1], device=dev()))
    with pytest.raises(ValueError, match='both None'):
        g0.without()


def test_samplers_walk_and_trending_on_an_erased_graph_equal_a_graph_from_scratch():
    from www2023tiger_amd import hip_ops
    N, E = 300, 4000
    ev = small_eids(events(stream(N, E, seed=5)))
    S, R = picks(N, ev, seed=2)
    parent = resident(N, ev, strategy='recent_edges', seed=5)
    child = parent.without(S, R)
    ref = graph_of(N, filtered(ev, S, R), strategy='recent_edges', seed=5)
    rs = np.random.RandomState(3)
    q_np = np.concatenate([rs.randint(0, N, 300), S[:20], ev[0][-100:]])
    t_np = np.concatenate([rs.uniform(0, ev[2][-1] + 2, 300), np.full(20, ev[2][-1] + 1), ev[2][-100:] + 1])
    q, qt = torch.from_numpy(q_np).to(dev()), torch.from_numpy(t_np).to(dev())
    for K in (1, 10):
        got, want = child.sample_device(q, qt, K), ref.sample_device(q, qt, K)
        for a, b, nm in zip(got, want, ('nbr', 'eid', 'ts', 'dir')):
            assert torch.equal(a, b), f'recent_edges K={K} {nm}'
        assert not np.isin(got[0].cpu().numpy(), S).any()
    assert bool((got[0] != 0).any())
    assert not torch.equal(parent.sample_device(q, qt, 10)[0], got[0])   # the parent still holds the erased entries
    for a, b in zip(child.get_history(q_np, t_np, 7), ref.get_history(q_np, t_np, 7)):
        np.testing.assert_array_equal(a, b)
    src = q[(q != 0)][:200]
    ts = qt[(q != 0)][:200]
    wa, wb = hip_ops.walk_candidates(child, src, ts, 32), hip_ops.walk_candidates(ref, src, ts, 32)
    for k in ('ids', 'counts', 'n_valid'):
        assert torch.equal(wa[k], wb[k]), f'walk_candidates {k}'
    assert int(wa['n_valid'].sum()) > 0 and not np.isin(wa['ids'].cpu().numpy(), S).any()
    assert np.isin(hip_ops.walk_candidates(parent, src, ts, 32)['ids'].cpu().numpy(), S).any()
    t_now = float(ev[2][-1]) + 1.0
    for window in (None, 200.0):
        ta, tb = hip_ops.trending(child, t_now, 64, window=window), hip_ops.trending(ref, t_now, 64, window=window)
        for k in ('ids', 'counts', 'n_valid', 'n_distinct'):
            assert torch.equal(ta[k], tb[k]), f'trending {k}'
        assert int(ta['n_valid']) > 0 and not np.isin(ta['ids'].cpu().numpy(), S).any()
    assert np.isin(hip_ops.trending(parent, t_now, 64)['ids'].cpu().numpy(), S).any()


def test_extended_and_trimmed_keep_working_on_an_erased_graph():
    from _append_ref import host_append
    from _trim_ref import host_trim
    N, E = 400, 3000
    s = small_eids(events(stream(N, E, seed=77)))
    part = lambda lo, hi: tuple(np.ascontiguousarray(a[lo:hi]) for a in s)
    S, R = picks(N, part(0, 1500), seed=4)
    g = resident(N, part(0, 1500)).without(S, R)
    h = host_erase(host_build(N, *part(0, 1500)), S, R)[1]
    assert_same(arrays(g), h, 'without')
    g2 = g.extended(*part(1500, 2200)).extended(*part(2200, E))   # erased ids come back as nodes never seen
    want = host_append(N, host_append(N, h, part(1500, 2200))[1], part(2200, E))[1]
    assert_same(arrays(g2), want, 'extended after without')
    assert np.diff(want[0])[S].any()
    assert_same(arrays(g2.trimmed(keep_last=3)), host_trim(want, -np.inf, 3)[1], 'trimmed after extended after without')
    assert_same(arrays(g2.without(S)), host_erase(want, S, None)[1], 'without twice')
    assert_same(g2._host_tcsr(), want, 'host view')
    with pytest.raises(ValueError, match='before the latest event'):
        g.extended(*part(0, 10))
