"""T-CSR extension on the GPU: Graph.extended / tg_tcsr_append against tg_tcsr_build_host over [old events | new events],
all four arrays bit for bit; sizes at the limits of the one-workgroup sort (2 n = 4096 entries) and of the copy tile (2048
old entries); nothing written outside the out arrays or into the parent; the samplers and the seen mask on an extended
graph against the same calls on a graph built from scratch."""
import ctypes as C

import numpy as np
import pytest
import torch

from _append_ref import CASES, NAMES, assert_same, cut, host_build, reference, stream

pytestmark = pytest.mark.gpu

AP_SMALL, AP_TILE = 4096, 2048   # tg_append.hip: entries the one-workgroup sort takes, old entries per copy block
GUARD = 0x5A


def dev():
    return torch.device('cuda', 0)


def graph_of(N, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    kw.setdefault('device', dev())
    return Graph.from_arrays(*ev, max_node_id=N - 1, **kw)


def arrays(g):
    return [t.cpu().numpy() for t in g._tensors()]


# the limits, +-1 event: 2 n = 4094 / 4096 / 4098 new entries, 2 E0 = 2046 / 2048 / 2050 and 4094 / 4096 / 4098 old entries
EDGES = {f'N400-E{E0}-n{n}': (400, E0, stream(400, E0 + n, seed=E0 + n))
         for E0, n in [(AP_TILE // 2 - 1, AP_SMALL // 2 - 1), (AP_TILE // 2, AP_SMALL // 2), (AP_TILE // 2 + 1, AP_SMALL // 2 + 1),
                       (AP_TILE - 1, 40), (AP_TILE, 1), (AP_TILE + 1, AP_SMALL // 2 - 1), (0, AP_SMALL // 2 + 1)]}
ALL = dict(CASES, **EDGES)


@pytest.mark.parametrize('case', list(ALL))
def test_extended_on_the_device_equals_the_host_build(case):
    N, old, new = cut(ALL[case])
    g0 = graph_of(N, old)
    before = arrays(g0)   # built on the device: the parent is device resident
    assert g0._dev is not None
    g1 = g0.extended(*new)
    assert g1._dev is not None and g1._log is not None   # extended on the device, no host view made
    assert_same(arrays(g1), reference(N, old, new), case)
    assert_same(arrays(g0), before, 'the parent is unchanged')
    assert g1.tcsr.num_entry == 2 * (len(old[0]) + len(new[0])) and g1.tcsr.serial == g1.serial != g0.serial
    # the lazily produced host view is the host builder's too
    assert_same(g1._host_tcsr(), reference(N, old, new), case + ' (host view)')
    assert_same(arrays(g1), g1._host_tcsr(), case)


def test_a_chain_on_the_device_and_device_tensor_inputs():
    N, E = 700, 9000
    s = stream(N, E, seed=71)
    cuts = [1000, 1001, 3050, 3050, 5200, E]   # one event, an empty batch, a batch past the one-workgroup limit
    g = h = graph_of(N, tuple(a[:cuts[0]] for a in s))
    g._tensors(), h._tensors()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        g = g.extended(*(a[lo:hi] for a in s))                                 # host inputs
        h = h.extended(*(t(a[lo:hi]) for a in s), validate=bool(i % 2))        # device inputs, checked and trusted
        assert_same(arrays(h), arrays(g), f'batch {i}')
    assert_same(arrays(g), host_build(N, *s), 'chain')
    assert_same(h._host_tcsr(), host_build(N, *s), 'chain, device inputs (host view)')
    assert len(h._events[0]) == E


def test_device_inputs_are_validated_with_one_read_back_and_refused_before_any_launch():
    N = 65
    s = stream(N, 300, seed=51)
    g = graph_of(N, tuple(a[:150] for a in s))
    before = arrays(g)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())

    def bad(col, idx, val):
        b = [a[150:].copy() for a in s]
        b[col][idx] = val
        return [t(a) for a in b]
    for col, idx, val, msg in ((2, 40, s[2][189] - 1, 'non-decreasing'), (2, 0, s[2][149] - 1, 'before the latest event'),
                               (0, 3, N, 'node ids'), (1, 3, -1, 'node ids'), (3, 3, 2 ** 31, '31 bits'), (3, 3, -1, '31 bits')):
        with pytest.raises(ValueError, match=msg):
            g.extended(*bad(col, idx, val))
    assert_same(arrays(g), before, 'nothing ran')


def raw_append(N, g_dev, new, *, ws_bytes=None):
    """tg_tcsr_append into out arrays with 64 guard bytes behind each -> (rc, [out arrays incl. guards as uint8 tensors])"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    d = dev()
    n, P0 = len(new[0]), g_dev[1].numel()
    P = P0 + 2 * n
    sizes = [(N + 1) * 8, P * 8, P * 4, P * 4]
    outs = [torch.full((sz + 64,), GUARD, dtype=torch.uint8, device=d) for sz in sizes]
    batch = [torch.from_numpy(a).to(d) for a in new]
    need = int(lib.tg_tcsr_append_workspace_bytes(P0, n, N))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=d)
    g = TgTcsr(N, P0, *(ptr(x) for x in g_dev))
    rc = lib.tg_tcsr_append(C.byref(g), n, *(ptr(b) for b in batch), *(ptr(o) for o in outs), ptr(ws), nbytes, stream_ptr(d))
    torch.cuda.synchronize()
    return rc, outs, sizes, need


@pytest.mark.parametrize('case', ['N65-E1-n200', 'hub-radix', 'N400-E1024-n2048', 'N400-E0-n2049', 'n0'])
def test_guard_words_behind_the_out_arrays_stay_intact(case):
    N, old, new = cut(ALL[case])
    g0 = graph_of(N, old)
    rc, outs, sizes, _ = raw_append(N, g0._tensors(), new)
    assert rc == 0
    want = reference(N, old, new)
    for o, sz, w, nm in zip(outs, sizes, want, NAMES):
        assert bool((o[sz:] == GUARD).all()), f'{nm}: bytes behind the array were written'
        np.testing.assert_array_equal(o[:sz].cpu().numpy(), w.view(np.uint8), err_msg=nm)


@pytest.mark.parametrize('case', ['N65-E1-n200', 'hub-radix'])
def test_a_short_workspace_is_refused_before_any_launch(case):
    from www2023tiger_amd import _lib
    N, old, new = cut(ALL[case])
    g0 = graph_of(N, old)
    need = raw_append(N, g0._tensors(), new)[3]
    assert need > 0
    for short in (0, need // 2, need - 256 - 16):
        rc, outs, _, _ = raw_append(N, g0._tensors(), new, ws_bytes=short)
        assert rc == _lib.TG_EWORKSPACE
        assert all(bool((o == GUARD).all()) for o in outs), 'something was launched'
    assert _lib.lib.tg_tcsr_append_workspace_bytes(100, 0, N) == 0


@pytest.mark.parametrize('strategy', ['recent_edges', 'recent_nodes', 'uniform'])
def test_samplers_and_seen_mask_on_an_extended_graph_equal_a_graph_from_scratch(strategy):
    from www2023tiger_amd import hip_ops
    N, old, new = cut('hub-one-workgroup')
    full = tuple(np.concatenate([a, b]) for a, b in zip(old, new))
    ext = graph_of(N, old, strategy=strategy, seed=5)
    ext._tensors()
    ext = ext.extended(*new)
    ref = graph_of(N, full, strategy=strategy, seed=5)
    rs = np.random.RandomState(3)
    q = torch.from_numpy(np.concatenate([rs.randint(0, N, 500), full[0][-200:], full[1][-200:]])).to(dev())
    qt = torch.from_numpy(np.concatenate([rs.uniform(0, full[2][-1] + 2, 500), full[2][-200:], full[2][-200:] + 1])).to(dev())
    for K in (1, 10):
        for _ in range(2):   # 'uniform': the second call continues the stream where the first left it, on both
            got, want = ext.sample_device(q, qt, K), ref.sample_device(q, qt, K)
            for a, b, nm in zip(got, want, ('nbr', 'eid', 'ts', 'dir')):
                assert torch.equal(a, b), f'{strategy} K={K} {nm}'
    assert bool((got[0] != 0).any())
    if strategy == 'recent_edges':
        cand = torch.arange(1, N, 3, device=dev())
        col_of = hip_ops.catalogue_index(cand, N)
        a = hip_ops.seen_mask(ext, q, qt, col_of, cand.numel())
        b = hip_ops.seen_mask(ref, q, qt, col_of, cand.numel())
        assert torch.equal(a, b) and not bool(a.all())
        old_only = hip_ops.seen_mask(graph_of(N, old), q, qt, col_of, cand.numel())
        assert not torch.equal(old_only, a)   # the new edges are seen


def test_uniform_draws_of_parent_and_child_continue_one_stream():
    N, old, new = cut('N65-E1-n200')
    full = tuple(np.concatenate([a, b]) for a, b in zip(old, new))
    twin = graph_of(N, full, strategy='uniform', seed=9)
    g0 = graph_of(N, tuple(a[:150] for a in full), strategy='uniform', seed=9)
    q = torch.arange(0, N, device=dev())
    qt = torch.full((N,), float(full[2][100]), dtype=torch.float64, device=dev())   # before the cut: both graphs agree
    a0, b0 = g0.sample_device(q, qt, 5), twin.sample_device(q, qt, 5)
    g1 = g0.extended(*(a[150:] for a in full))
    assert g1._mt is g0._mt and g1.rng is g0.rng
    a1, b1 = g1.sample_device(q, qt, 5), twin.sample_device(q, qt, 5)
    for x, y in zip(a0 + a1, b0 + b1):
        assert torch.equal(x, y)
