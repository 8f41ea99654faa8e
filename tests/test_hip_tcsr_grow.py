"""Node growth of the T-CSR on the GPU: tg_tcsr_append_grow / Graph.extended(num_node=) / Graph.widened against the host twin
(which tests/test_tcsr_grow_host.py holds against tg_tcsr_build_host with the larger node count), all four arrays bit for
bit: the cases of the host test, node counts around the block width of the indptr write, the radix path where the key widens
from 12 to 16 bits; nothing written outside the out arrays or into the parent; the old entry gives the bits it gave."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _grow_ref as R

pytestmark = pytest.mark.gpu

GUARD = 0x5A
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'www2023tiger_amd', 'csrc', 'tg_append.hip')


def constant(name):
    m = re.search(r'constexpr int %s = (\d+);' % name, open(SRC).read())
    assert m, name
    return int(m.group(1))


AP_THREADS, AP_SMALL = constant('AP_THREADS'), constant('AP_SMALL')


def dev():
    return torch.device('cuda', 0)


def graph_of(N, ev):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(*ev, strategy='recent_edges', seed=0, max_node_id=N - 1, device=dev())


def arrays(g):
    return [t.cpu().numpy() for t in g._tensors()]


def host_twin(N0, N1, old, new):
    rc, want = R.host_append_grow(N0, N1, R.host_build(N0, *old), new)
    assert rc == 0
    return want


# indptr_out has N1 + 1 entries, written AP_THREADS to a block: N1 + 1 at one and two blocks, +-1, from below and across
_W = AP_THREADS


def straddle(a, b):
    N0, N1, old, new = R.grow_case(a, b, 300, 200, seed=a + b, frac_new=0.2)
    new[0][-1] = new[1][7] = N1 - 1   # the largest id does appear, as a source and as a destination
    return N0, N1, old, new


STRADDLE = {f'N{a}-to-{b}': straddle(a, b)
            for a, b in [(_W - 3, _W - 2), (_W - 2, _W - 1), (_W - 1, _W), (_W - 2, _W + 1), (2 * _W - 2, 2 * _W - 1),
                         (2 * _W - 1, 2 * _W), (_W - 1, 2 * _W + 1), (_W, 2 * _W - 2)]}


def key_widens(n):
    """4096 nodes sort on 12 key bits, 4097 on 16: 40 of the n new events are owned by node 4096 on either side (they sort
    last), spread over the batch"""
    N0, N1, old, new = R.grow_case(4096, 4097, 3000, n, seed=77 + n, frac_new=0.0)
    new = tuple(a.copy() for a in new)
    at = np.linspace(0, n - 1, 40).astype(np.int64)
    new[0][at[::2]] = 4096
    new[1][at[1::2]] = 4096
    new[1][at[0]] = 4096   # a self loop on the new node
    return N0, N1, old, new


WIDEN = {'key-12-to-16-radix': key_widens(AP_SMALL // 2 + 1), 'key-12-to-16-one-workgroup': key_widens(AP_SMALL // 2),
         'key-12-to-16-small': key_widens(100)}
ALL = dict(R.CASES, **STRADDLE, **WIDEN)


def test_the_cases_take_the_paths_they_are_named_for():
    assert 2 * len(WIDEN['key-12-to-16-radix'][3][0]) == AP_SMALL + 2 and 2 * len(WIDEN['key-12-to-16-one-workgroup'][3][0]) == AP_SMALL
    for c in WIDEN.values():
        assert int(np.sum(c[3][0] == 4096) + np.sum(c[3][1] == 4096)) >= 40 and c[2][0].max() < 4096
    for c in STRADDLE.values():
        assert max(c[3][0].max(), c[3][1].max()) == c[1] - 1   # the largest new id does appear


def raw_grow(N0, N1, g_dev, new, entry='grow'):
    """tg_tcsr_append_grow (or the old entry) into out arrays with 64 guard bytes behind each -> (rc, outs, sizes)"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    d = dev()
    n, P0 = len(new[0]), g_dev[1].numel()
    P = P0 + 2 * n
    sizes = [(N1 + 1) * 8, P * 8, P * 4, P * 4]
    outs = [torch.full((sz + 64,), GUARD, dtype=torch.uint8, device=d) for sz in sizes]
    batch = [torch.from_numpy(a).to(d) for a in new]
    need = int(lib.tg_tcsr_append_grow_workspace_bytes(P0, n, N0, N1))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=d)
    g = TgTcsr(N0, P0, *(ptr(x) for x in g_dev))
    tail = (*(ptr(b) for b in batch), *(ptr(o) for o in outs), ptr(ws), need, stream_ptr(d))
    if entry == 'grow':
        rc = lib.tg_tcsr_append_grow(C.byref(g), N1, n, *tail)
    else:
        assert N0 == N1
        rc = lib.tg_tcsr_append(C.byref(g), n, *tail)
    torch.cuda.synchronize()
    return rc, outs, sizes


@pytest.mark.parametrize('case', list(ALL))
def test_the_device_entry_equals_the_host_twin_and_writes_nothing_else(case):
    N0, N1, old, new = ALL[case]
    g0 = graph_of(N0, old)
    before = arrays(g0)
    rc, outs, sizes = raw_grow(N0, N1, g0._tensors(), new)
    assert rc == 0
    want = host_twin(N0, N1, old, new)
    for o, sz, w, nm in zip(outs, sizes, want, R.NAMES):
        assert bool((o[sz:] == GUARD).all()), f'{nm}: bytes behind the array were written'
        np.testing.assert_array_equal(o[:sz].cpu().numpy(), w.view(np.uint8), err_msg=f'{case} {nm}')
    R.assert_same(arrays(g0), before, 'the parent is unchanged')


@pytest.mark.parametrize('case', list(ALL))
def test_extended_on_the_device_with_num_node(case):
    N0, N1, old, new = ALL[case]
    g0 = graph_of(N0, old)
    before = arrays(g0)
    assert g0._dev is not None
    g1 = g0.extended(*new, num_node=N1)
    assert g1._dev is not None and g1._log is not None and g1.num_node == N1 and g0.num_node == N0
    want = host_twin(N0, N1, old, new)
    R.assert_same(arrays(g1), want, case)
    R.assert_same(arrays(g1), R.reference(N1, old, new), case + ' (the build with N1 nodes)')
    R.assert_same(arrays(g0), before, 'the parent is unchanged')
    assert g1.tcsr.num_node == N1 and g0.tcsr.num_node == N0 and g1._mt_state() is g0._mt_state() and g1.rng is g0.rng
    R.assert_same(g1._host_tcsr(), want, case + ' (host view)')   # produced lazily, from a root that covers fewer ids


def test_the_old_entry_forwards_and_gives_todays_bits():
    N0, _, old, new = R.CASES['no-growth']
    g0 = graph_of(N0, old)
    a = raw_grow(N0, N0, g0._tensors(), new, entry='old')
    b = raw_grow(N0, N0, g0._tensors(), new)
    assert a[0] == 0 and b[0] == 0
    for x, y, sz, w in zip(a[1], b[1], a[2], R.reference(N0, old, new)):
        assert torch.equal(x, y)
        np.testing.assert_array_equal(x[:sz].cpu().numpy(), w.view(np.uint8))


@pytest.mark.parametrize('how', ['trimmed', 'renumbered'])
def test_growth_after_trimmed_and_after_renumbered_on_the_device(how):
    """a graph trimmed / renumbered ON THE DEVICE (its host origin is its device arrays) extended with a larger count: the
    device arrays and the lazily produced host view - downloaded with the old count, extended by the host twin with the
    new one - against the build over the kept events followed by the new ones with N1 nodes"""
    N0, N1, old, new = R.CASES['N255-to-257']
    old = (old[0], old[1], old[2], np.arange(1, len(old[0]) + 1, dtype=np.int64))
    parent = graph_of(N0, old)
    parent._tensors()
    if how == 'trimmed':
        t_cut = float(old[2][len(old[2]) // 2])
        mid = parent.trimmed(before=t_cut)
        kept = tuple(a[old[2] >= t_cut] for a in old)
    else:
        remap = torch.arange(len(old[0]) + 1, dtype=torch.int32, device=dev())   # the identity numbering
        mid = parent.renumbered(remap, parent._dev[3].clone())
        kept = old
    assert mid._dev is not None and mid._root.dev is not None and mid.num_node == N0
    before = arrays(mid)
    child = mid.extended(*new, num_node=N1)
    assert child._dev is not None and child.num_node == N1 and child._dev[0].numel() == N1 + 1
    want = R.reference(N1, kept, new)
    R.assert_same(arrays(child), want, how)
    R.assert_same(child._host_tcsr(), want, how + ' (host view)')
    R.assert_same(arrays(mid), before, 'the parent is unchanged')
    assert len(mid._host_tcsr()[0]) == N0 + 1   # ... and so is its host view: the download covers the old count
    auto = mid.extended(*(torch.from_numpy(a).to(dev()) for a in new), num_node='auto')
    assert auto.num_node == N1
    R.assert_same(arrays(auto), want, how + ' (auto, device inputs)')


def test_a_chain_with_auto_device_inputs_widened_trimmed_and_renumbered():
    N0, N1, old, new = R.grow_case(100, 140, 500, 900, seed=91, frac_new=0.05)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    g = graph_of(N0, old)
    g._tensors()
    cuts = [0, 1, 300, 300, 900]
    seen = N0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = tuple(a[lo:hi] for a in new)
        g = g.extended(*(t(a) for a in part), num_node='auto')   # the maximum comes from the validation's one read-back
        if hi > lo:
            seen = max(seen, int(max(part[0].max(), part[1].max())) + 1)
        assert g.num_node == seen and g._dev[0].numel() == seen + 1
    R.assert_same(arrays(g), R.reference(seen, old, new), 'chain')
    R.assert_same(g._host_tcsr(), R.reference(seen, old, new), 'chain (host view)')
    with pytest.raises(ValueError, match='auto'):
        g.extended(*(t(a) for a in R.CASES['gap'][3]), num_node='auto', validate=False)
    far = tuple(a.copy() for a in new)
    far[2][:] += 1e6
    trusted = g.extended(*(t(a[:5]) for a in far), num_node=seen + 7, validate=False)   # an explicit count is trusted
    assert trusted.num_node == seen + 7
    wide = g.widened(seen + 300)
    assert wide.num_node == seen + 300 and wide._dev is not None
    R.assert_same(arrays(wide), R.reference(seen + 300, old, new), 'widened')
    assert g.num_node == seen
    cutoff = float(new[2][400])
    trimmed = wide.trimmed(before=cutoff)
    assert trimmed.num_node == seen + 300 and trimmed._dev[0].numel() == seen + 301
    ren = wide.renumbered(None, wide._dev[3].clone())
    assert ren.num_node == seen + 300
    again = trimmed.extended(*(t(a[:5]) for a in far))
    assert again.num_node == seen + 300
    with pytest.raises(ValueError, match='does not grow'):
        again.extended(t(np.array([seen + 300])), t(np.array([1])), t(np.array([2e6])), t(np.array([5])))
