"""Node-id compaction without a GPU: the host twins (tg_node_compact_plan_host, tg_node_rows_compact_host,
tg_bitmap_compact_host), Graph.compacted on host graphs and IdMap('cpu').compact against the reference of
_node_compact_ref.py (numpy, a dict, from_arrays over the remapped events)."""
import numpy as np
import pytest
import torch

from _node_compact_ref import (DROPS, OWN_SIZES, SIZES, bitmap, bitmap_compact_ref, compacted_ref, drop_ids, events, graph_of,
                               remap_ref, unpack)
from www2023tiger_amd import hip_ops
from www2023tiger_amd._lib import TigerHipError
from www2023tiger_amd.data.idmap import IdMap

INT64_MIN = -(1 << 63)


def host_case(N, name, num_node=None):
    num_node = N if num_node is None else num_node
    drop = drop_ids(N, name)
    ev = events(num_node, drop)
    return drop, ev, graph_of(ev, num_node)


@pytest.mark.parametrize('name', DROPS)
@pytest.mark.parametrize('N', SIZES + OWN_SIZES)
def test_plan_and_compacted_graph_equal_the_reference(N, name):
    drop, ev, g = host_case(N, name)
    before = [a.copy() for a in g._host_tcsr()]
    plan = hip_ops.node_compact_host(g, bitmap(drop, N))
    remap, old_of = remap_ref(N, drop)
    assert np.array_equal(plan.remap.numpy(), remap) and np.array_equal(plan.old_of.numpy(), old_of)
    assert (plan.n_old, plan.n_new, plan.n_graph_old, plan.n_graph_new) == (N, len(old_of), N, len(old_of))
    assert int(plan.remap[0]) == 0 and plan.code == 0
    child = g.compacted(plan)
    got, ref = child._host_tcsr(), compacted_ref(ev, remap, plan.n_graph_new)
    for a, b, what in zip(got, ref, ('indptr', 'ts', 'nbr', 'eid')):
        assert a.dtype == b.dtype and np.array_equal(a, b), f'N={N} {name}: {what}'
    assert child.num_node == plan.n_new and child.serial != g.serial and child.rng is g.rng
    assert got[1] is g._host_tcsr()[1] and got[3] is g._host_tcsr()[3], 'ts and eid are shared with the parent'
    for a, b in zip(g._host_tcsr(), before):
        assert np.array_equal(a, b), 'the parent is only read'
    if len(ev[0]):   # the child is still the T-CSR of an event list: it extends like any graph
        t = float(ev[2][-1]) + 1.0
        a = int(old_of[-1])
        ext = child.extended([remap[a]], [remap[a]], [t], [len(ev[0]) + 1])
        ext_ref = graph_of(tuple(np.concatenate([x, y]) for x, y in zip(
            (remap[ev[0]].astype(np.int64), remap[ev[1]].astype(np.int64), ev[2], ev[3]),
            (np.array([remap[a]], dtype=np.int64), np.array([remap[a]], dtype=np.int64), np.array([t]), np.array([len(ev[0]) + 1])))),
            plan.n_new)
        for x, y in zip(ext._host_tcsr(), ext_ref._host_tcsr()):
            assert np.array_equal(x, y)


@pytest.mark.parametrize('N,num_node', [(65, 64), (140000, 131073), (2049, 1), (513, 512)])
def test_ids_beyond_the_graph_are_kept_or_dropped_like_any_other(N, num_node):
    drop = drop_ids(N, 'edges' if N > 65 else 'last')
    drop = np.union1d(drop, [N - 1])
    ev = events(num_node, drop)
    g = graph_of(ev, num_node)
    plan = hip_ops.node_compact_host(g, bitmap(drop, N), N)
    remap, old_of = remap_ref(N, drop)
    assert np.array_equal(plan.remap.numpy(), remap) and np.array_equal(plan.old_of.numpy(), old_of)
    n_graph = int((old_of < num_node).sum())
    assert (plan.n_new, plan.n_graph_old, plan.n_graph_new) == (len(old_of), num_node, n_graph)
    assert plan.rows_below(num_node) == n_graph and plan.rows_below(N) == len(old_of) and plan.rows_below(1) == 1
    for a, b in zip(g.compacted(plan)._host_tcsr(), compacted_ref(ev, remap, n_graph)):
        assert np.array_equal(a, b)


def test_hub_rows_next_to_thousands_of_empty_rows():
    N = 140000
    drop = np.arange(2, 131070)          # a run of dropped, empty rows between two hubs
    rs = np.random.RandomState(1)
    E = 5000
    src = np.where(rs.rand(E) < 0.5, 1, 131070).astype(np.int64)
    dst = np.where(rs.rand(E) < 0.7, 131071, rs.randint(131072, N, E)).astype(np.int64)
    ev = (src, dst, np.arange(E, dtype=np.float64), np.arange(1, E + 1, dtype=np.int64))
    g = graph_of(ev, N)
    assert np.diff(g._host_tcsr()[0]).max() > 1000
    plan = hip_ops.node_compact_host(g, bitmap(drop, N))
    remap, _ = remap_ref(N, drop)
    for a, b in zip(g.compacted(plan)._host_tcsr(), compacted_ref(ev, remap, plan.n_new)):
        assert np.array_equal(a, b)


def test_every_error_class_names_its_smallest_offender():
    N = 300
    ev = events(N, np.zeros(0, dtype=np.int64), E=400)
    g = graph_of(ev, N)
    h = g._host_tcsr()
    deg = np.diff(h[0])
    # ID0
    plan = hip_ops.node_compact_host(g, bitmap([0, 5], N), strict=False)
    assert (plan.code, plan.first) == (1, 0)
    with pytest.raises(ValueError, match='ID0: node id 0 is the padding id'):
        hip_ops.node_compact_host(g, bitmap([0], N))
    # SPARE: bits at or beyond N in the last word; two of them: the smaller
    plan = hip_ops.node_compact_host(g, bitmap([310, 305], N, words=5), strict=False)
    assert (plan.code, plan.first) == (2, 305)
    # ROW: two dropped ids that own entries: the smaller
    owners = np.nonzero(deg > 0)[0]
    owners = owners[owners > 0]
    a, b = int(owners[3]), int(owners[7])
    plan = hip_ops.node_compact_host(g, bitmap([b, a], N), strict=False)
    assert (plan.code, plan.first) == (3, a)
    with pytest.raises(ValueError, match=f'ROW: node {a} is dropped but still owns entries of the graph: erase it first'):
        hip_ops.node_compact_host(g, bitmap([b, a], N))
    # NBR: the owner's row is empty (a graph `without` its rows alone), its id still stands as a neighbour: the smallest entry
    keep = np.repeat(np.arange(N), deg) != a
    ind = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(N), deg)[keep], minlength=N))]).astype(np.int64)
    g2 = g._child()._adopt_host((ind, h[1][keep].copy(), h[2][keep].copy(), h[3][keep].copy()), None, g)
    first = int(np.nonzero(g2._host_tcsr()[2] == a)[0][0])
    plan = hip_ops.node_compact_host(g2, bitmap([a], N), strict=False)
    assert (plan.code, plan.first) == (4, first)
    with pytest.raises(ValueError, match=f'NBR: entry {first} of the graph names a dropped node'):
        hip_ops.node_compact_host(g2, bitmap([a], N))
    with pytest.raises(ValueError, match='compacted: NBR'):
        g2.compacted(plan)
    # the classes are reported in the order ID0, SPARE, ROW, NBR
    plan = hip_ops.node_compact_host(g2, bitmap([0, a, 310], N, words=5), strict=False)
    assert (plan.code, plan.first) == (1, 0)
    plan = hip_ops.node_compact_host(g, bitmap([a, 310], N, words=5), strict=False)
    assert (plan.code, plan.first) == (2, 310)
    assert hip_ops.NODE_COMPACT_TEXT(0) == 'a clean compaction plan'


def test_argument_errors():
    g = graph_of(events(100, np.array([99]), E=50), 100)
    with pytest.raises(ValueError, match='n_ids = 99'):
        hip_ops.node_compact_host(g, bitmap([], 100), 99)
    with pytest.raises(ValueError, match='drop_bits over 100 ids'):
        hip_ops.node_compact_host(g, bitmap([], 64))
    with pytest.raises(ValueError, match='drop_bits over 100 ids'):
        hip_ops.node_compact_host(g, bitmap([], 100).astype(np.int32))
    plan = hip_ops.node_compact_host(g, bitmap([99], 100))
    other = graph_of(events(90, np.zeros(0, dtype=np.int64), E=50), 90)
    with pytest.raises(ValueError, match='the plan covers a graph of 100 nodes, this graph has 90'):
        other.compacted(plan)
    with pytest.raises(ValueError, match='an id outside'):
        plan.translate(torch.tensor([100]))
    assert plan.translate(torch.tensor([0, 98, 99], dtype=torch.int32)).tolist() == [0, 98, -1]
    assert plan.translate(torch.tensor([[1, 99]])).dtype == torch.int64
    assert hip_ops.node_compact_host(None, bitmap([3], 10), 10).old_of.tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9]


ROW_SHAPES = [((), torch.uint8), ((), torch.float32), ((), torch.float64), ((), torch.int64), ((4,), torch.float32),
              ((8,), torch.float32), ((172,), torch.float32), ((256,), torch.float32), ((2, 2), torch.float64)]


def rows_tables(n_src, n_out, seed=0):
    """one (src, dst, reference rows) per row shape; every table its own row count"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (shape, dt) in enumerate(ROW_SHAPES):
        rows = max(1, n_src - 3 * i)   # tables of different row counts in one call
        src = torch.randint(0, 250, (rows,) + shape, generator=g).to(dt)
        out.append((src, rows))
    return out


@pytest.mark.parametrize('N', [1, 2, 65, 2049, 4099, 140000])
def test_rows_compaction_equals_a_numpy_gather(N):
    drop = drop_ids(N, 'alternating')
    plan = hip_ops.node_compact_host(None, bitmap(drop, N), N)
    tabs = rows_tables(N, plan.n_new)
    for lo in (0, 8):   # at most 8 tables per call
        pairs, refs = [], []
        for src, rows in tabs[lo:lo + 8]:
            n_out = plan.rows_below(rows)
            dst = torch.zeros((n_out + 2,) + tuple(src.shape[1:]), dtype=src.dtype)   # a backing store with head-room
            pairs.append((src, dst[:n_out]))
            refs.append((dst, src[plan.old_of[:n_out].long()]))
        hip_ops.node_rows_compact(pairs, plan.old_of)
        for dst, ref in refs:
            assert torch.equal(dst[:len(ref)], ref) and not dst[len(ref):].any(), 'rows beyond n_out are not written'


def test_rows_compaction_refusals():
    plan = hip_ops.node_compact_host(None, bitmap([2], 10), 10)
    src = torch.arange(40, dtype=torch.float32).reshape(10, 4)
    nine = [(src, torch.zeros(9, 4)) for _ in range(9)]
    with pytest.raises(ValueError, match='9 tables in one call'):
        hip_ops.node_rows_compact(nine, plan.old_of)
    hip_ops.node_rows_compact(nine[:8], plan.old_of)
    assert all(torch.equal(d, src[plan.old_of.long()]) for _, d in nine[:8])
    with pytest.raises(ValueError, match='rows of 12 bytes'):
        hip_ops.node_rows_compact([(torch.zeros(10, 3), torch.zeros(9, 3))], plan.old_of)
    with pytest.raises(ValueError, match='rows of 2 bytes'):
        hip_ops.node_rows_compact([(torch.zeros(10, dtype=torch.int16), torch.zeros(9, dtype=torch.int16))], plan.old_of)
    with pytest.raises(ValueError, match='wants 10 rows, old_of has 9'):
        hip_ops.node_rows_compact([(src, torch.zeros(10, 4))], plan.old_of)
    with pytest.raises(ValueError, match='one dtype and row shape'):
        hip_ops.node_rows_compact([(src, torch.zeros(9, 8))], plan.old_of)
    with pytest.raises(TigerHipError, match='invalid argument'):   # src and dst overlap
        hip_ops.node_rows_compact([(src, src[1:])], plan.old_of)
    hip_ops.node_rows_compact([], plan.old_of)


@pytest.mark.parametrize('N', [1, 63, 64, 65, 129, 2049, 140000])
def test_bitmap_compaction_and_zero_spare_bits(N):
    rs = np.random.RandomState(N)
    drop = drop_ids(N, 'edges') if N > 65 else drop_ids(N, 'one')
    plan = hip_ops.node_compact_host(None, bitmap(drop, N), N)
    ids = np.nonzero(rs.rand(N) < 0.5)[0]
    bits = bitmap(ids, N)
    got = plan.bitmap(torch.from_numpy(bits))
    assert np.array_equal(got.numpy(), bitmap_compact_ref(bits, N, plan.old_of.numpy()))
    assert got.numel() == hip_ops.bitmap_words(plan.n_new)
    assert not unpack(got.numpy(), 64 * got.numel())[plan.n_new:].any(), 'spare bits are zero'
    full = plan.bitmap(torch.full((len(bits),), -1, dtype=torch.int64))   # every old bit set, the spare ones too
    assert unpack(full.numpy(), 64 * full.numel()).sum() == plan.n_new
    n_in = max(1, N - 70)   # a bitmap over fewer ids: a model that admitted fewer than the map assigned
    part = plan.bitmap(torch.from_numpy(bitmap(ids[ids < n_in], n_in)), n_in)
    assert np.array_equal(part.numpy(), bitmap_compact_ref(bits, n_in, plan.old_of.numpy()))
    with pytest.raises(ValueError, match='words for'):
        plan.bitmap(torch.zeros(len(bits), dtype=torch.int64), N + 1)


def churned_map(keys_n=200, capacity=16):
    m = IdMap('cpu', capacity)
    keys = torch.arange(1000, 1000 + keys_n, dtype=torch.int64) * 7919
    ids = m.assign(keys)
    d = dict(zip(keys.tolist(), ids.tolist()))
    return m, keys, d


def test_idmap_compact_shrinks_capacity_and_keeps_the_mapping():
    m, keys, d = churned_map()
    caps = [m.capacity]
    live = keys
    for _ in range(4):   # the pinned sequence: 201 ids -> 512 slots, then 101 -> 256, 51 -> 128, 26 -> 64, 13 -> 32
        gone = live[::2].contiguous()
        _, removed = m.remove(gone)
        old_size, old_key_of, free = m.size, m.key_of[:m.size].clone(), m.free_ids()
        assert removed.numel() == gone.numel() and m.n_free == gone.numel()
        plan = m.compact()
        remap, old_of = remap_ref(old_size, free.numpy())
        assert np.array_equal(plan.remap.numpy(), remap) and np.array_equal(plan.old_of.numpy(), old_of)
        live = live[1::2].contiguous()
        assert (m.size, m.n_free, m.slots_used) == (live.numel() + 1, 0, live.numel() + 1)
        assert not m.free_bits.any() and m.free_ids().numel() == 0
        got = m.lookup(keys)
        want = torch.tensor([int(remap[d[k]]) if k in set(live.tolist()) else -1 for k in keys.tolist()], dtype=torch.int32)
        assert torch.equal(got, want), 'lookup of a live key gives remap[old id], of a removed key -1'
        assert torch.equal(m.key_of[:m.size], old_key_of[plan.old_of.long()])
        d = {k: int(remap[d[k]]) for k in live.tolist()}
        caps.append(m.capacity)
    assert caps == [512, 256, 128, 64, 32]
    # assign afterwards hands out size, size + 1, ...; a removed key that comes back is a new key
    size = m.size
    new = torch.tensor([5, int(keys[0]), 6, 5], dtype=torch.int64)
    assert m.assign(new).tolist() == [size, size + 1, size + 2, size]
    # the state round trip is version 1
    sd = m.state_dict()
    assert sd['format'] == 'tiger-idmap' and sd['version'] == 1 and set(sd) == {'format', 'version', 'key_of'}
    back = IdMap.from_state_dict(sd, 'cpu')
    assert torch.equal(back.lookup(keys), m.lookup(keys)) and back.size == m.size


def test_idmap_compact_edges():
    m, keys, d = churned_map(20)
    plan = m.compact()   # nothing free: the identity plan, nothing changes
    assert plan.identity and m.size == 21 and torch.equal(m.lookup(keys), torch.arange(1, 21, dtype=torch.int32))
    table = m.slot_key
    assert m.compact().identity and m.slot_key is table
    m.remove(keys)       # everything but the padding id leaves
    plan = m.compact()
    assert (m.size, m.n_free, m.capacity, plan.n_new) == (1, 0, 16, 1)
    assert m.lookup(keys).eq(-1).all() and m.assign(keys[:3]).tolist() == [1, 2, 3]
    assert int(m.key_of[0]) == INT64_MIN
    # a plan that is not this map's is refused and nothing changes
    m.remove(keys[:1])
    wrong = hip_ops.node_compact_host(None, bitmap([], m.size), m.size)
    before = (m.size, m.n_free, m.slot_key)
    with pytest.raises(ValueError, match='IdMap.compact: the plan covers'):
        m.compact(wrong)
    assert (m.size, m.n_free, m.slot_key) == before
