"""T-CSR trim on the GPU: Graph.trimmed / tg_tcsr_trim_plan + tg_tcsr_trim_apply on a device-resident parent against the
host twin (which tests/test_tcsr_trim_host.py holds against numpy and against the build over the filtered events), all
four arrays bit for bit; node counts at the seams of the plan's 256-node chunks (and past 256 chunks, where a workgroup
strides over the chunk totals), kept totals at the seams of the 2048-entry copy tile, tiles whose owner window exceeds
the LDS window, a hub row over many tiles; nothing written outside the out arrays or into the parent; the samplers and
the seen mask on a trimmed graph against a graph built from scratch; guarantee (b).

The plan's node kernels and the copy kernel launch one workgroup per chunk / tile (tg_trim.hip: `cdiv(g->num_node,
TR_THREADS)`, `cdiv(num_entry_out, TR_TILE)`): no grid is capped, so there is no size past a cap to test."""
import ctypes as C

import numpy as np
import pytest
import torch

from _append_ref import NAMES, assert_same, host_build, stream
from _trim_ref import STREAMS, events, host_trim, trim_by_build, trims_of

pytestmark = pytest.mark.gpu

TR_CHUNK, TR_TILE, TR_WIN = 256, 2048, 2048   # tg_trim.hip: TR_THREADS (nodes per plan workgroup), TR_TILE, TR_WIN
GUARD = 0x5A


def dev():
    return torch.device('cuda', 0)


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


def dense_then_sparse():
    """1500 events among nodes [0, 50), then 200 among [50, 6000): the first copy tile lies inside a few dense rows (its
    window is staged in LDS), the second one runs from the dense rows over thousands of mostly empty ones"""
    rs = np.random.RandomState(12)
    src = np.concatenate([rs.randint(0, 50, 1500), rs.randint(50, 6000, 200)]).astype(np.int64)
    dst = np.concatenate([rs.randint(0, 50, 1500), rs.randint(50, 6000, 200)]).astype(np.int64)
    return src, dst, np.floor(np.sort(rs.uniform(0, 500, 1700))), rs.randint(0, 2 ** 31, 1700).astype(np.int64)


GPU_STREAMS = dict(STREAMS, **{
    'hub-10-tiles': (300, stream(300, 12000, seed=8, hub=7)),
    'dense-then-sparse': (6000, dense_then_sparse()),
    f'N{TR_CHUNK * 257 + 3}-E1000': (TR_CHUNK * 257 + 3, stream(TR_CHUNK * 257 + 3, 1000, seed=9)),   # 258 chunks
})
GPU_STREAMS.update({f'N{N}-E600': (N, stream(N, 600, seed=N))
                    for N in (TR_CHUNK - 1, TR_CHUNK, TR_CHUNK + 1, 2 * TR_CHUNK, 2 * TR_CHUNK + 1)})


def trims_for(name, ev):
    if name in STREAMS:
        return trims_of(name)
    t = float(np.median(ev[2]))
    return [('copy', -np.inf, None), ('median', t, None), ('keep2', -np.inf, 2), ('median+keep3', t, 3),
            ('keep0', -np.inf, 0), ('above-all', float(ev[2].max()) + 1, None)]


@pytest.mark.parametrize('name', list(GPU_STREAMS))
def test_trimmed_on_the_device_equals_the_host_twin(name):
    N, s = GPU_STREAMS[name]
    ev = events(s)
    g0 = resident(N, ev)
    before = arrays(g0)
    h = host_build(N, *ev)
    assert_same(before, h, 'the parent')
    for label, t_cut, keep_last in trims_for(name, ev):
        g1 = g0.trimmed(before=None if t_cut == -np.inf else t_cut, keep_last=keep_last)
        rc, want, kept = host_trim(h, t_cut, -1 if keep_last is None else keep_last)
        assert rc == 0
        got = arrays(g1)
        assert_same(got, want, f'{name} {label}')
        assert g1.tcsr.num_entry == kept == g1._dev[1].numel() and g1.tcsr.serial == g1.serial != g0.serial
        assert g1._dev[1].untyped_storage().nbytes() == 8 * kept   # allocated exactly
        if keep_last is None:
            assert_same(got, trim_by_build(N, ev, t_cut), f'{name} {label} (build over the filtered events)')
        assert_same(g1._host_tcsr(), want, f'{name} {label} (host view)')
    assert_same(arrays(g0), before, 'the parent is unchanged')


def test_the_cases_reach_the_paths_they_are_named_for():
    """owner windows beyond the LDS window (one tile of a two-tile copy, and a single sparse tile), a hub over ten tiles"""
    N, s = GPU_STREAMS['dense-then-sparse']
    indptr = host_build(N, *events(s))[0]
    owner = lambda q: int(np.searchsorted(indptr, q, 'right')) - 1
    P = int(indptr[-1])
    assert TR_TILE < P <= 2 * TR_TILE
    assert owner(TR_TILE - 1) - owner(0) <= TR_WIN < owner(P - 1) - owner(TR_TILE)
    N, s = GPU_STREAMS['N9228-E300']
    indptr = host_build(N, *events(s))[0]
    assert int(np.searchsorted(indptr, indptr[-1] - 1, 'right')) - int(np.searchsorted(indptr, 0, 'right')) > TR_WIN
    N, s = GPU_STREAMS['hub-10-tiles']
    indptr = host_build(N, *events(s))[0]
    assert indptr[8] - indptr[7] > 10 * TR_TILE


@pytest.mark.parametrize('total', [TR_TILE - 1, TR_TILE, TR_TILE + 1, 2 * TR_TILE, 2 * TR_TILE + 1])
def test_kept_totals_at_the_seams_of_the_copy_tile(total):
    """node 0 is the source of every event, the destinations cycle over ten nodes, times are distinct: a horizon that
    keeps k events leaves k entries on node 0 and k on the others, a cap M < k then leaves M + k"""
    E, D = 3000, 10
    ev = (np.zeros(E, dtype=np.int64), 1 + np.arange(E, dtype=np.int64) % D, np.arange(E, dtype=np.float64),
          np.arange(E, dtype=np.int64))
    k = total // 2 + 50
    M = total - k
    assert k // D + 1 <= M < k
    g1 = resident(D + 1, ev).trimmed(before=float(E - k), keep_last=M)
    rc, want, kept = host_trim(host_build(D + 1, *ev), float(E - k), M)
    assert rc == 0 and kept == total
    assert_same(arrays(g1), want, f'total {total}')


def raw_trim(g_dev, N, t_cut, keep_last, *, ws_bytes=None, entries=None):
    """plan + read-back + apply into out arrays with 64 guard bytes behind each -> (rc of plan, rc of apply, outs, sizes)"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    d = dev()
    need = int(lib.tg_tcsr_trim_workspace_bytes(N))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.full((need,), GUARD, dtype=torch.uint8, device=d)
    g = TgTcsr(N, g_dev[1].numel(), *(ptr(x) for x in g_dev))
    indptr = torch.full(((N + 1) * 8 + 64,), GUARD, dtype=torch.uint8, device=d)
    rc_plan = lib.tg_tcsr_trim_plan(C.byref(g), t_cut, keep_last, ptr(indptr), ptr(ws), nbytes, stream_ptr(d))
    torch.cuda.synchronize()
    if rc_plan != 0:
        return rc_plan, None, [indptr, ws], need
    P = int(indptr[:(N + 1) * 8].view(torch.int64)[-1]) if entries is None else entries
    sizes = [(N + 1) * 8, P * 8, P * 4, P * 4]
    outs = [indptr] + [torch.full((sz + 64,), GUARD, dtype=torch.uint8, device=d) for sz in sizes[1:]]
    rc_apply = lib.tg_tcsr_trim_apply(C.byref(g), ptr(indptr), P, *(ptr(o) for o in outs[1:]), ptr(ws), nbytes, stream_ptr(d))
    torch.cuda.synchronize()
    return rc_plan, rc_apply, outs, sizes


@pytest.mark.parametrize('name,t_cut,keep_last', [('N65-E201', 30.0, 3), ('hub', -np.inf, 128), ('N9228-E300', 40.0, -1),
                                                  ('dense-then-sparse', 100.0, 64), ('tiny', np.inf, -1), ('tiny', 1.0, 0)])
def test_guard_bytes_behind_the_out_arrays_stay_intact(name, t_cut, keep_last):
    N, s = GPU_STREAMS[name]
    ev = events(s)
    g0 = resident(N, ev)
    rc_plan, rc_apply, outs, sizes = raw_trim(g0._tensors(), N, t_cut, keep_last)
    assert rc_plan == 0 and rc_apply == 0
    _, want, kept = host_trim(host_build(N, *ev), t_cut, keep_last)
    assert sizes[1] == 8 * kept
    for o, sz, w, nm in zip(outs, sizes, want, NAMES):
        assert bool((o[sz:] == GUARD).all()), f'{nm}: bytes behind the array were written'
        np.testing.assert_array_equal(o[:sz].cpu().numpy(), w.view(np.uint8), err_msg=nm)


def test_a_short_workspace_and_a_nan_are_refused_before_any_launch():
    from www2023tiger_amd import _lib
    N, s = GPU_STREAMS['N1000-E2048']
    g0 = resident(N, events(s))
    need = int(_lib.lib.tg_tcsr_trim_workspace_bytes(N))
    assert need >= 8 * N
    for short in (0, need // 2, need - 1):
        rc, _, (indptr, ws), _ = raw_trim(g0._tensors(), N, 100.0, 5, ws_bytes=short)
        assert rc == _lib.TG_EWORKSPACE
        assert bool((indptr == GUARD).all()) and bool((ws == GUARD).all()), 'something was launched'
    rc, _, (indptr, ws), _ = raw_trim(g0._tensors(), N, float('nan'), 5)
    assert rc == _lib.TG_EINVAL and bool((indptr == GUARD).all()) and bool((ws == GUARD).all())
    # apply: a short workspace, and an entry count that no trim of this graph can have
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    rc_plan, rc_apply, outs, sizes = raw_trim(g0._tensors(), N, 100.0, 5)
    assert rc_plan == 0 and rc_apply == 0
    g = TgTcsr(N, g0._dev[1].numel(), *(ptr(x) for x in g0._dev))
    fresh = [torch.full((sz + 64,), GUARD, dtype=torch.uint8, device=dev()) for sz in sizes[1:]]
    ws = torch.zeros(need, dtype=torch.uint8, device=dev())
    P = sizes[1] // 8
    assert lib.tg_tcsr_trim_apply(C.byref(g), ptr(outs[0]), P, *(ptr(o) for o in fresh), ptr(ws), need - 1,
                                  stream_ptr(dev())) == _lib.TG_EWORKSPACE
    for bad in (-1, g.num_entry + 1):
        assert lib.tg_tcsr_trim_apply(C.byref(g), ptr(outs[0]), bad, *(ptr(o) for o in fresh), ptr(ws), need,
                                      stream_ptr(dev())) == _lib.TG_EINVAL
    torch.cuda.synchronize()
    assert all(bool((o == GUARD).all()) for o in fresh), 'something was launched'


@pytest.mark.parametrize('strategy', ['recent_edges', 'recent_nodes', 'uniform'])
def test_samplers_and_seen_mask_on_a_trimmed_graph_equal_a_graph_from_scratch(strategy):
    from www2023tiger_amd import hip_ops
    N, s = GPU_STREAMS['hub']
    ev = events(s)
    t_cut = float(np.median(ev[2]))
    kept_ev = tuple(np.ascontiguousarray(a[ev[2] >= t_cut]) for a in ev)
    parent = resident(N, ev, strategy=strategy, seed=5)
    trm = parent.trimmed(before=t_cut)
    assert trm._mt is parent._mt and trm.rng is parent.rng
    ref = graph_of(N, kept_ev, strategy=strategy, seed=5)
    rs = np.random.RandomState(3)
    q = torch.from_numpy(np.concatenate([rs.randint(0, N, 500), ev[0][-200:], ev[1][-200:]])).to(dev())
    qt = torch.from_numpy(np.concatenate([rs.uniform(0, ev[2][-1] + 2, 500), ev[2][-200:], ev[2][-200:] + 1])).to(dev())
    for K in (1, 10):
        for _ in range(2):   # 'uniform': the second call continues the stream where the first left it, on both
            got, want = trm.sample_device(q, qt, K), ref.sample_device(q, qt, K)
            for a, b, nm in zip(got, want, ('nbr', 'eid', 'ts', 'dir')):
                assert torch.equal(a, b), f'{strategy} K={K} {nm}'
    assert bool((got[0] != 0).any())
    if strategy == 'recent_edges':
        cand = torch.arange(1, N, 3, device=dev())
        col_of = hip_ops.catalogue_index(cand, N)
        a = hip_ops.seen_mask(trm, q, qt, col_of, cand.numel())
        b = hip_ops.seen_mask(ref, q, qt, col_of, cand.numel())
        assert torch.equal(a, b) and not bool(a.all())
        assert not torch.equal(hip_ops.seen_mask(parent, q, qt, col_of, cand.numel()), a)   # the dropped edges were seen


def test_the_last_keep_last_entries_serve_every_query_past_the_latest_time():
    """guarantee (b): parent and keep_last = M child agree on recent_edges K = M and get_history H = M at every time later
    than the graph's latest event - and not for K = M + 1, so the agreement is no accident of short rows"""
    N, s = GPU_STREAMS['N65-E201']
    ev = events(s)
    M = 4
    parent = resident(N, ev, strategy='recent_edges', seed=0)
    child = parent.trimmed(keep_last=M)
    assert int(np.diff(arrays(parent)[0]).max()) > M + 1 and int(np.diff(arrays(child)[0]).max()) == M
    q = torch.arange(N, device=dev()).repeat(2)
    qt = torch.cat([torch.full((N,), float(ev[2][-1]) + 0.5, dtype=torch.float64),
                    torch.full((N,), float(ev[2][-1]) + 1e6, dtype=torch.float64)]).to(dev())
    for K in (1, M):
        for a, b in zip(child.sample_device(q, qt, K), parent.sample_device(q, qt, K)):
            assert torch.equal(a, b), K
    for a, b in zip(child.get_history(q.cpu().numpy(), qt.cpu().numpy(), M), parent.get_history(q.cpu().numpy(), qt.cpu().numpy(), M)):
        np.testing.assert_array_equal(a, b)
    more_c, more_p = child.sample_device(q, qt, M + 1), parent.sample_device(q, qt, M + 1)
    assert bool((more_c[0] != more_p[0]).any(1).any())
    assert torch.equal(more_c[0][:, 1:], more_p[0][:, 1:])   # (the child lacks exactly the oldest slot)


def test_extended_to_and_the_host_view_keep_working_on_a_trimmed_graph():
    N, E = 400, 3000
    s = events(stream(N, E, seed=77))
    part = lambda lo, hi: tuple(np.ascontiguousarray(a[lo:hi]) for a in s)
    g = resident(N, part(0, 1500)).trimmed(before=float(s[2][700]), keep_last=6)
    assert g._events is None and g._log is None
    dev_arrays = arrays(g)
    h = host_trim(host_build(N, *part(0, 1500)), float(s[2][700]), 6)[1]
    assert_same(dev_arrays, h, 'trimmed')
    assert_same(g._host_tcsr(), dev_arrays, 'the host view is the device arrays')
    # a chain on the device behind a trimmed graph, then its host view (the trimmed arrays extended on the host)
    g2 = g.extended(*part(1500, 2200)).extended(*part(2200, E))
    assert g2._dev is not None and g2._log is not None
    from _append_ref import host_append
    want = host_append(N, host_append(N, h, part(1500, 2200))[1], part(2200, E))[1]
    assert_same(arrays(g2), want, 'extended after trimmed')
    g3 = g2.trimmed(keep_last=3)   # a trim of a chain whose root was trimmed: no host view is needed for it
    assert g2._log is not None
    assert_same(arrays(g3), host_trim(want, -np.inf, 3)[1], 'trimmed after extended after trimmed')
    assert_same(g2._host_tcsr(), want, 'extended after trimmed (host view)')
    with pytest.raises(ValueError, match='before the latest event'):
        g3.extended(*part(0, 10))
    # .to(): the device arrays are dropped and come back from the host view
    fresh = resident(N, part(0, 1500)).trimmed(keep_last=6)
    kept = arrays(fresh)
    fresh.to('cpu')
    assert fresh._dev is None
    fresh.to(dev())
    assert_same(arrays(fresh), kept, 'after to()')
    child = resident(N, part(0, 1500)).trimmed(keep_last=6).extended(*part(1500, 2200))
    kept = arrays(child)
    child.to('cpu').to(dev())
    assert_same(arrays(child), kept, 'a child of a trimmed graph after to()')
    assert int(child.extended(*part(2200, E)).tcsr.num_entry) == len(kept[1]) + 2 * (E - 2200)
