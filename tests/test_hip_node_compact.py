"""Node-id compaction on the device: tg_node_compact_plan, tg_node_rows_compact, tg_bitmap_compact, Graph.compacted on
device-resident graphs and IdMap.compact - the cases of test_node_compact_host.py through the kernels, against the
reference of _node_compact_ref.py AND the host twins, with torch.equal."""
import numpy as np
import pytest
import torch

from _node_compact_ref import (DROPS, OWN_SIZES, SIZES, bitmap, bitmap_compact_ref, compacted_ref, drop_ids, events, graph_of,
                               remap_ref, unpack)
from test_node_compact_host import ROW_SHAPES, rows_tables
from www2023tiger_amd import hip_ops
from www2023tiger_amd._lib import TigerHipError
from www2023tiger_amd.data.graph import Graph
from www2023tiger_amd.data.idmap import IdMap

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def dev_bits(ids, n_ids, words=None):
    return torch.from_numpy(bitmap(ids, n_ids, words)).to(DEV)


def same_plan(p, h, what):
    assert torch.equal(p.remap.cpu(), h.remap) and torch.equal(p.old_of.cpu(), h.old_of), what
    assert (p.n_old, p.n_new, p.n_graph_old, p.n_graph_new, p.code, p.first) == \
        (h.n_old, h.n_new, h.n_graph_old, h.n_graph_new, h.code, h.first), what


def check_case(N, name, num_node=None):
    num_node = N if num_node is None else num_node
    drop = drop_ids(N, name)
    if num_node < N:
        drop = np.union1d(drop, [N - 1])
    ev = events(num_node, drop)
    host = graph_of(ev, num_node)
    g = graph_of(ev, num_node).to(DEV)
    parent = [t.clone() for t in g._tensors()]
    plan = hip_ops.node_compact_plan(g, dev_bits(drop, N), N)
    what = f'N={N} {name} num_node={num_node}'
    same_plan(plan, hip_ops.node_compact_host(host, bitmap(drop, N), N), what)
    remap, old_of = remap_ref(N, drop)
    assert np.array_equal(plan.remap.cpu().numpy(), remap) and np.array_equal(plan.old_of.cpu().numpy(), old_of), what
    child = g.compacted(plan)
    ref = compacted_ref(ev, remap, plan.n_graph_new)
    for a, b, arr in zip(child._dev, ref, ('indptr', 'ts', 'nbr', 'eid')):
        assert torch.equal(a.cpu(), torch.from_numpy(b)), f'{what}: {arr}'
    assert child._dev[1] is g._dev[1] and child._dev[3] is g._dev[3], 'ts and eid are shared with the parent'
    assert child.num_node == plan.n_graph_new and child.tcsr.num_node == plan.n_graph_new and child.rng is g.rng
    assert child._mt_state() is g._mt_state() and child.serial != g.serial
    for a, b in zip(g._dev, parent):
        assert torch.equal(a, b), 'the parent is only read'
    code, first, _ = hip_ops.tcsr_verify(child)
    assert code == 0, hip_ops.TCSR_VERIFY_TEXT(code, first)


@pytest.mark.parametrize('N', SIZES + OWN_SIZES)
def test_plan_and_compacted_graph_equal_reference_and_host_twin(N):
    for name in DROPS:
        check_case(N, name)


@pytest.mark.parametrize('N,num_node', [(65, 64), (140000, 131073), (2049, 1), (513, 512), (262149, 131072)])
def test_ids_beyond_the_graph(N, num_node):
    for name in ('last', 'edges', 'alternating'):
        check_case(N, name, num_node)


def test_hub_rows_next_to_thousands_of_empty_rows():
    N = 140000
    drop = np.arange(2, 131070)
    rs = np.random.RandomState(1)
    E = 5000
    src = np.where(rs.rand(E) < 0.5, 1, 131070).astype(np.int64)
    dst = np.where(rs.rand(E) < 0.7, 131071, rs.randint(131072, N, E)).astype(np.int64)
    ev = (src, dst, np.arange(E, dtype=np.float64), np.arange(1, E + 1, dtype=np.int64))
    g = graph_of(ev, N).to(DEV)
    plan = hip_ops.node_compact_plan(g, dev_bits(drop, N))
    remap, _ = remap_ref(N, drop)
    for a, b in zip(g.compacted(plan)._tensors(), compacted_ref(ev, remap, plan.n_new)):
        assert torch.equal(a.cpu(), torch.from_numpy(b))


def test_every_error_class_names_its_smallest_offender():
    """offenders in DIFFERENT workgroups (ids 131 072 apart, entries 2 048 apart): the smaller one whatever ran first"""
    N = 140000
    ev = events(N, np.zeros(0, dtype=np.int64), E=6000)
    host = graph_of(ev, N)
    g = graph_of(ev, N).to(DEV)
    h = host._host_tcsr()
    deg = np.diff(h[0])

    def both(graph, hgraph, ids, words=None):
        p = hip_ops.node_compact_plan(graph, dev_bits(ids, N, words), N, strict=False)
        same_plan(p, hip_ops.node_compact_host(hgraph, bitmap(ids, N, words), N, strict=False), str(ids))
        return p.code, p.first

    assert both(g, host, [0, 5]) == (1, 0)
    with pytest.raises(ValueError, match='ID0: node id 0 is the padding id'):
        hip_ops.node_compact_plan(g, dev_bits([0], N))
    W = (N + 63) // 64
    assert both(g, host, [N + 9, N + 3], W) == (2, N + 3)
    owners = np.nonzero(deg > 0)[0]
    a, b = int(owners[owners > 0][2]), int(owners[owners > 131072][-1])
    assert both(g, host, [b, a]) == (3, a)
    with pytest.raises(ValueError, match=f'ROW: node {a} is dropped but still owns entries of the graph: erase it first'):
        hip_ops.node_compact_plan(g, dev_bits([b, a], N))
    # NBR: the rows of a and b are emptied, their ids still stand as neighbours in other rows
    owner = np.repeat(np.arange(N), deg)
    keep = (owner != a) & (owner != b)
    ind = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=N))]).astype(np.int64)
    arrays = (ind, h[1][keep].copy(), h[2][keep].copy(), h[3][keep].copy())
    hosts2 = host._child()._adopt_host(arrays, None, host)
    g2 = Graph._from_device_arrays(tuple(torch.from_numpy(x).to(DEV) for x in arrays), g._t_last, True)
    named = np.nonzero(np.isin(arrays[2], [a, b]))[0]
    assert named[-1] - named[0] > 2048, 'the offenders must lie in different workgroups'
    assert both(g2, hosts2, [a, b]) == (4, int(named[0]))
    with pytest.raises(ValueError, match=f'NBR: entry {int(named[0])} of the graph names a dropped node'):
        hip_ops.node_compact_plan(g2, dev_bits([a, b], N))
    assert both(g2, hosts2, [0, a, N + 1], W) == (1, 0)
    assert both(g, host, [a, N + 1], W) == (2, N + 1)
    # a neighbour that is no id of the graph indexes nothing and is reported
    bad = [t.clone() for t in g._tensors()]
    bad[2][7] = N + 5
    bad[2][3000] = -4
    g3 = Graph._from_device_arrays(tuple(bad), g._t_last, True)
    p = hip_ops.node_compact_plan(g3, dev_bits([], N), N, strict=False)
    assert (p.code, p.first) == (4, 7)


def test_argument_errors_before_any_launch():
    N = 100
    g = graph_of(events(N, np.array([99]), E=50), N).to(DEV)
    with pytest.raises(ValueError, match='n_ids = 99'):
        hip_ops.node_compact_plan(g, dev_bits([], N), 99)
    with pytest.raises(ValueError, match='drop_bits over 100 ids'):
        hip_ops.node_compact_plan(g, dev_bits([], 64))
    with pytest.raises(ValueError, match='runs on the device'):
        hip_ops.node_compact_plan(g, torch.zeros(2, dtype=torch.int64))
    # the C entry: a short workspace is TG_EWORKSPACE, a misaligned one and a missing array TG_EINVAL
    import ctypes as C
    from www2023tiger_amd._lib import TG_EINVAL, TG_EWORKSPACE, lib, ptr
    t = g.tcsr
    bits = dev_bits([], N)
    remap, old_of = (torch.empty(N, dtype=torch.int32, device=DEV) for _ in range(2))
    indptr, nbr = torch.empty(N + 1, dtype=torch.int64, device=DEV), torch.empty(t.num_entry, dtype=torch.int32, device=DEV)
    out4 = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    need = int(lib.tg_node_compact_workspace_bytes(N))
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    st = hip_ops.stream_ptr(torch.device(DEV))
    call = lambda *a: lib.tg_node_compact_plan(C.byref(t), ptr(bits), bits.numel(), *a, st)
    assert call(N, ptr(remap), ptr(old_of), ptr(indptr), ptr(nbr), ptr(out4), ptr(ws), need - 1) == TG_EWORKSPACE
    assert call(N, ptr(remap), ptr(old_of), ptr(indptr), ptr(nbr), ptr(out4), ptr(ws) + 8, need) == TG_EINVAL
    assert call(N, None, ptr(old_of), ptr(indptr), ptr(nbr), ptr(out4), ptr(ws), need) == TG_EINVAL
    assert call(N - 1, ptr(remap), ptr(old_of), ptr(indptr), ptr(nbr), ptr(out4), ptr(ws), need) == TG_EINVAL
    assert lib.tg_node_compact_workspace_bytes(0) == 0 and lib.tg_node_compact_workspace_bytes(1 << 31) == 0
    torch.cuda.synchronize()
    assert out4.tolist() == [-7] * 4, 'nothing was launched'
    assert call(N, ptr(remap), ptr(old_of), ptr(indptr), ptr(nbr), ptr(out4), ptr(ws), need) == 0
    assert out4.tolist() == [N, N, 0, -1]


@pytest.mark.parametrize('N', [1, 2, 65, 2049, 4099, 140000])
def test_rows_compaction_equals_index_select_and_host_twin(N):
    drop = drop_ids(N, 'alternating' if N != 4099 else 'edges')
    plan = hip_ops.node_compact_plan(None, dev_bits(drop, N), N)
    hplan = hip_ops.node_compact_host(None, bitmap(drop, N), N)
    tabs = rows_tables(N, plan.n_new)
    assert len(tabs) == len(ROW_SHAPES) == 9
    for lo in (0, 8):   # at most 8 tables per call
        pairs, hpairs, refs = [], [], []
        for src, rows in tabs[lo:lo + 8]:
            n_out = plan.rows_below(rows)
            d_src = src.to(DEV)
            dst = torch.zeros((n_out + 2,) + tuple(src.shape[1:]), dtype=src.dtype, device=DEV)
            hdst = torch.zeros((n_out,) + tuple(src.shape[1:]), dtype=src.dtype)
            pairs.append((d_src, dst[:n_out]))
            hpairs.append((src, hdst))
            refs.append((dst, hdst, d_src.index_select(0, plan.old_of[:n_out].long())))
        hip_ops.node_rows_compact(pairs, plan.old_of)
        hip_ops.node_rows_compact(hpairs, hplan.old_of)
        for dst, hdst, ref in refs:
            assert torch.equal(dst[:len(ref)], ref) and torch.equal(dst[:len(ref)].cpu(), hdst)
            assert not dst[len(ref):].any(), 'rows beyond n_out are not written'


def test_rows_compaction_refusals():
    plan = hip_ops.node_compact_plan(None, dev_bits([2], 10), 10)
    src = torch.arange(40, dtype=torch.float32, device=DEV).reshape(10, 4)
    nine = [(src, torch.zeros(9, 4, device=DEV)) for _ in range(9)]
    with pytest.raises(ValueError, match='9 tables in one call'):
        hip_ops.node_rows_compact(nine, plan.old_of)
    hip_ops.node_rows_compact(nine[:8], plan.old_of)
    assert all(torch.equal(d, src[plan.old_of.long()]) for _, d in nine[:8])
    with pytest.raises(ValueError, match='rows of 12 bytes'):
        hip_ops.node_rows_compact([(torch.zeros(10, 3, device=DEV), torch.zeros(9, 3, device=DEV))], plan.old_of)
    with pytest.raises(TigerHipError, match='invalid argument'):   # src and dst overlap
        hip_ops.node_rows_compact([(src, src[1:])], plan.old_of)
    wide = torch.zeros(11, 5, dtype=torch.float32, device=DEV).reshape(-1)[1:41].reshape(10, 4)   # 4 bytes off a 16-byte line
    with pytest.raises(TigerHipError, match='invalid argument'):
        hip_ops.node_rows_compact([(wide, torch.zeros(9, 4, device=DEV))], plan.old_of)
    with pytest.raises(ValueError, match='on cuda'):
        hip_ops.node_rows_compact([(src.cpu(), torch.zeros(9, 4))], plan.old_of)


@pytest.mark.parametrize('N', [1, 63, 64, 65, 129, 2049, 140000])
def test_bitmap_compaction_and_zero_spare_bits(N):
    rs = np.random.RandomState(N)
    drop = drop_ids(N, 'edges') if N > 65 else drop_ids(N, 'one')
    plan = hip_ops.node_compact_plan(None, dev_bits(drop, N), N)
    hplan = hip_ops.node_compact_host(None, bitmap(drop, N), N)
    ids = np.nonzero(rs.rand(N) < 0.5)[0]
    bits = bitmap(ids, N)
    got = plan.bitmap(torch.from_numpy(bits).to(DEV))
    assert torch.equal(got.cpu(), hplan.bitmap(torch.from_numpy(bits)))
    assert np.array_equal(got.cpu().numpy(), bitmap_compact_ref(bits, N, plan.old_of.cpu().numpy()))
    assert got.numel() == hip_ops.bitmap_words(plan.n_new)
    full = plan.bitmap(torch.full((len(bits),), -1, dtype=torch.int64, device=DEV))   # every old bit set, the spare ones too
    assert unpack(full.cpu().numpy(), 64 * full.numel()).sum() == plan.n_new, 'spare bits are zero'
    n_in = max(1, N - 70)
    part = plan.bitmap(torch.from_numpy(bitmap(ids[ids < n_in], n_in)).to(DEV), n_in)
    assert np.array_equal(part.cpu().numpy(), bitmap_compact_ref(bits, n_in, plan.old_of.cpu().numpy()))
    assert torch.equal(plan.translate(torch.arange(N, device=DEV)).cpu(), hplan.remap.long())


def test_idmap_compact_equals_the_host_twin_and_shrinks():
    maps = [IdMap(DEV, 16), IdMap('cpu', 16)]
    keys = torch.arange(1000, 4000, dtype=torch.int64) * 7919
    for m in maps:
        m.assign(keys.to(m.device))
    caps, live = [maps[0].capacity], keys
    for _ in range(4):
        gone, live = live[::3].contiguous(), torch.cat([live[1::3], live[2::3]]).sort().values
        plans = []
        for m in maps:
            m.remove(gone.to(m.device))
            old_size, free = m.size, m.free_ids()
            plans.append(m.compact())
            remap, old_of = remap_ref(old_size, free.numpy())
            assert np.array_equal(plans[-1].remap.cpu().numpy(), remap) and np.array_equal(plans[-1].old_of.cpu().numpy(), old_of)
        d, h = maps
        assert (d.size, d.n_free, d.slots_used, d.capacity) == (h.size, h.n_free, h.slots_used, h.capacity)
        assert d.size == live.numel() + 1 and not d.free_bits.any()
        assert torch.equal(d.key_of[:d.size].cpu(), h.key_of[:h.size])
        assert torch.equal(d.lookup(keys.to(DEV)).cpu(), h.lookup(keys))
        assert int((d.lookup(keys.to(DEV)) > 0).sum()) == live.numel()
        caps.append(d.capacity)
    assert caps == [8192, 4096, 4096, 2048, 2048]   # 3001 ids, then 2001, 1334, 889, 593
    size = maps[0].size
    assert maps[0].assign(torch.tensor([5, int(keys[0]), 5], device=DEV)).tolist() == [size, size + 1, size]
    sd = maps[0].state_dict()
    assert sd['format'] == 'tiger-idmap' and sd['version'] == 1
    back = IdMap.from_state_dict(sd, DEV)
    assert torch.equal(back.lookup(keys.to(DEV)), maps[0].lookup(keys.to(DEV)))
