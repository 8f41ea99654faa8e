"""Node growth without a GPU: tg_tcsr_append_grow_host (and Graph.extended(num_node=) / Graph.widened on host-only graphs)
against tg_tcsr_build_host over [old events | new events] with the LARGER node count - all four arrays, bit for bit -, and
the growth of the per-node tables (Memory.grow, MessageStoreNoGradLastOnly.grow, NumericalFeature.append_node_rows) on CPU
tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import _grow_ref as R

TG_EINVAL = -1


def graph_of(N, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(*ev, strategy='recent_edges', seed=0, max_node_id=N - 1, device='cpu', **kw)


def host_arrays(g):
    return g._host_tcsr()


# ------------------------------------------------------------------------------------------------------ the C entries
@pytest.mark.parametrize('case', list(R.CASES))
def test_host_twin_equals_the_build_over_the_concatenated_stream_with_the_larger_count(case):
    N0, N1, old, new = R.CASES[case]
    rc, got = R.host_append_grow(N0, N1, R.host_build(N0, *old), new)
    assert rc == 0
    want = R.reference(N1, old, new)
    R.assert_same(got, want, case)
    assert len(got[0]) == N1 + 1 and got[0][-1] == 2 * (len(old[0]) + len(new[0]))


def test_the_old_host_entry_forwards_and_gives_todays_bits():
    N0, N1, old, new = R.CASES['no-growth']
    h = R.host_build(N0, *old)
    rc, got = R.host_append_grow(N0, N0, h, new)
    from _append_ref import host_append
    rc0, got0 = host_append(N0, h, new)
    assert rc == 0 and rc0 == 0
    R.assert_same(got, got0, 'forwarding')
    R.assert_same(got0, R.reference(N0, old, new), 'old entry')


def test_every_einval_of_the_new_entries():
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    N0, N1, old, new = R.CASES['gap']
    h = R.host_build(N0, *old)
    assert R.host_append_grow(N0, N0 - 1, h, R.EMPTY)[0] == TG_EINVAL            # num_node_out < num_node
    assert R.host_append_grow(N0, 0x80000000, h, R.EMPTY)[0] == TG_EINVAL        # num_node_out > 2^31 - 1
    assert R.host_append_grow(N0, N0 + 5, h, new)[0] == TG_EINVAL                # id N0 + 5 == num_node_out
    assert R.host_append_grow(N0, N0 + 6, h, new)[0] == 0
    neg = tuple(a.copy() for a in new)
    neg[1][0] = -1
    assert R.host_append_grow(N0, N1, h, neg)[0] == TG_EINVAL
    # the device entry validates its arguments before it touches the device (ids are the host twin's to check)
    g = TgTcsr(N0, len(h[1]), *(ptr(a) for a in h))
    out = [np.empty(N1 + 1, dtype=np.int64)] + [np.empty(len(h[1]), dtype=dt) for dt in (np.float64, np.int32, np.int32)]
    for bad in (N0 - 1, 0x80000000):
        assert lib.tg_tcsr_append_grow(C.byref(g), bad, 0, None, None, None, None, *(ptr(a) for a in out), None, 0,
                                       None) == TG_EINVAL
        assert lib.tg_tcsr_append_grow_workspace_bytes(len(h[1]), 10, N0, bad) == 0
    assert lib.tg_tcsr_append_grow_workspace_bytes(len(h[1]), 10, N0, N1) == lib.tg_tcsr_append_workspace_bytes(len(h[1]), 10, N0)
    assert lib.tg_tcsr_append_grow_workspace_bytes(len(h[1]), 0, N0, N1) == 0     # a pure widening needs no workspace


# ------------------------------------------------------------------------------------------------------------- Graph
@pytest.mark.parametrize('case', list(R.CASES))
def test_graph_extended_with_num_node_on_a_host_only_graph(case):
    N0, N1, old, new = R.CASES[case]
    parent = graph_of(N0, old)
    before = tuple(a.copy() for a in host_arrays(parent))
    child = parent.extended(*new, num_node=N1)
    assert child.num_node == N1 and parent.num_node == N0 and child.rng is parent.rng
    R.assert_same(host_arrays(child), R.reference(N1, old, new), case)
    R.assert_same(host_arrays(parent), before, 'the parent')
    # a further batch on the grown graph keeps its count
    again = child.extended(*R.EMPTY)
    assert again.num_node == N1
    R.assert_same(host_arrays(again), R.reference(N1, old, new), 'extended again')


def test_an_unordered_root_keeps_its_own_count_when_a_child_grows():
    """the host builder path (events out of time order): the child's view must not widen the arrays its parent shares"""
    N0, N1, old, new = R.hand_case(20, 23, 60, [22, 1], [3, 22])
    old = tuple(a.copy() for a in old)
    old[2][[3, 40]] = old[2][[40, 3]]   # out of order: from_arrays takes the host builder
    parent = graph_of(N0, old)
    assert not parent._time_ordered
    child = parent.extended(*new, num_node=N1)
    R.assert_same(host_arrays(child), R.reference(N1, old, new), 'child')
    assert len(host_arrays(parent)[0]) == N0 + 1


def test_auto_takes_the_largest_id_and_never_shrinks():
    N0, N1, old, new = R.CASES['gap']
    parent = graph_of(N0, old)
    child = parent.extended(*new, num_node='auto')
    assert child.num_node == N0 + 6
    R.assert_same(host_arrays(child), R.reference(N0 + 6, old, new), 'auto')
    same = child.extended(*R.EMPTY, num_node='auto')
    assert same.num_node == N0 + 6
    low = tuple(a.copy() for a in new)
    low[0][:] = 1
    low[1][:] = 2
    low[2][:] += 100.0
    assert child.extended(*low, num_node='auto').num_node == N0 + 6
    with pytest.raises(ValueError, match='num_node'):
        parent.extended(*new, num_node='largest')


def test_widened_is_extended_with_no_events():
    N0, N1, old, _ = R.CASES['no-events']
    parent = graph_of(N0, old)
    wide = parent.widened(N1)
    assert wide.num_node == N1 and parent.num_node == N0 and wide._t_last == parent._t_last
    R.assert_same(host_arrays(wide), R.host_build(N1, *old), 'widened')
    assert parent.widened(N0).num_node == N0
    with pytest.raises(ValueError, match='below'):
        parent.widened(N0 - 1)
    with pytest.raises(ValueError, match='31 bits'):
        parent.widened(2 ** 31)


def test_without_num_node_an_unknown_id_is_refused_with_todays_text():
    N0, N1, old, new = R.CASES['gap']
    parent = graph_of(N0, old)
    with pytest.raises(ValueError) as e:
        parent.extended(*new)
    assert str(e.value) == ("node ids must lie in [0, num_node) (num_node does not grow: the model's tables are sized by it)")
    with pytest.raises(ValueError, match='node ids must lie'):
        parent.extended(*new, num_node=N0 + 5)     # the id N0 + 5 itself is not below it


@pytest.mark.parametrize('how', ['trimmed', 'renumbered'])
def test_growth_after_trimmed_and_after_renumbered_and_they_keep_the_count(how):
    N0, N1, old, new = R.CASES['N255-to-257']
    old = (old[0], old[1], old[2], np.arange(1, len(old[0]) + 1, dtype=np.int64))
    parent = graph_of(N0, old)
    if how == 'trimmed':
        t_cut = float(old[2][len(old[2]) // 2])
        mid = parent.trimmed(before=t_cut)
        kept = tuple(a[old[2] >= t_cut] for a in old)
    else:
        h = host_arrays(parent)
        remap = np.arange(len(old[0]) + 1, dtype=np.int32)   # the identity numbering: the entries are what they were
        mid = parent.renumbered(remap, h[3].copy())
        kept = old
    child = mid.extended(*new, num_node=N1)
    R.assert_same(host_arrays(child), R.reference(N1, kept, new), how)
    # ... and both keep the count of a grown graph
    assert child.trimmed(before=float(new[2][0])).num_node == N1
    assert len(host_arrays(child.trimmed(keep_last=3))[0]) == N1 + 1
    assert child.renumbered(None, host_arrays(child)[3].copy()).num_node == N1


# ------------------------------------------------------------------------------------------------- the per-node tables
def filled_memory(n, d, seed=0):
    from www2023tiger_amd.model.memory import Memory
    m = Memory(n, d)
    g = torch.Generator().manual_seed(seed)
    m.vals.copy_(torch.randn(n, d, generator=g))
    m.update_ts.copy_(torch.rand(n, generator=g))
    m.active_mask.copy_(torch.rand(n, generator=g) < 0.5)
    return m


def test_memory_grow_within_capacity_and_past_it():
    m = filled_memory(10, 4)
    old = {k: v.clone() for k, v in m.state_dict().items()}
    v0 = m._version_
    p0 = m.vals.data_ptr()
    assert m.grow(12, reserve=20) is True and m.vals.data_ptr() != p0      # no backing store yet: the first growth moves
    p1 = (m.vals.data_ptr(), m.update_ts.data_ptr(), m.active_mask.data_ptr())
    assert m.grow(20) is False                                             # within capacity: nothing moves
    assert (m.vals.data_ptr(), m.update_ts.data_ptr(), m.active_mask.data_ptr()) == p1
    assert m.grow(20) is False and m.n == 20
    assert m.grow(21) is True and m.vals.data_ptr() != p1[0]               # past it: a new store, half as large again
    assert m._stores['vals'].shape[0] == 20 + 16 and m._version_ == v0 + 4
    sd = m.state_dict()
    assert list(sd) == ['vals', 'update_ts', 'active_mask']
    assert sd['vals'].shape == (21, 4) and sd['update_ts'].shape == (21,) and sd['active_mask'].shape == (21,)
    for k in sd:
        assert torch.equal(sd[k][:10], old[k]) and not bool(sd[k][10:].any()), k
    with pytest.raises(ValueError, match='never released'):
        m.grow(20)
    with pytest.raises(ValueError, match='reserve'):
        m.grow(30, reserve=29)
    assert m.n == 21 and m.vals.shape[0] == 21


def test_a_grown_memory_round_trips_through_a_state_dict_into_one_born_big():
    from www2023tiger_amd.model.memory import Memory
    m = filled_memory(10, 4)
    m.grow(33)
    big = Memory(33, 4)
    big.load_state_dict(m.state_dict())
    for k, v in big.state_dict().items():
        assert torch.equal(v, m.state_dict()[k]), k
    back = filled_memory(10, 4, seed=9)
    back.grow(33)
    back.load_state_dict(big.state_dict())
    assert torch.equal(back.vals, m.vals)


def test_a_table_that_was_replaced_gets_a_new_store():
    m = filled_memory(10, 4)
    m.grow(12, reserve=40)
    m.vals = m.vals.clone()            # what .to() does: the buffer no longer heads its store
    want = m.vals.clone()
    assert m.grow(13) is True
    assert torch.equal(m.vals[:12], want) and not bool(m.vals[12:].any())
    assert m.update_ts.data_ptr() == m._stores['update_ts'].data_ptr()


@pytest.mark.parametrize('n', [63, 64, 65, 128])
def test_mailbox_grow_and_the_word_count_of_its_bitmap(n):
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.model.memory import MessageStoreNoGradLastOnly
    n0 = 61
    s = MessageStoreNoGradLastOnly(n0, 6)
    g = torch.Generator().manual_seed(n)
    s.node_msg_vals.copy_(torch.randn(n0, 6, generator=g))
    s.node_msg_ts.copy_(torch.rand(n0, generator=g))
    s.has_msg_bits[0] = (1 << n0) - 1                                  # every node holds a message: bits 0 .. 60
    assert int(s.has_msg_bits[0]) >> n0 == 0                           # the spare bits of the old last word are zero
    v0 = s._version_
    assert s.grow(n) is True
    words = (n + 63) // 64
    assert hip_ops.bitmap_words(n) == words and s.has_msg_bits.shape == (words,) and s.has_msg_bits.dtype == torch.int64
    assert s.n == n and s._version_ == v0 + 1
    assert s.node_msg_vals.shape == (n, 6) and s.node_msg_ts.shape == (n,)
    assert not bool(s.node_msg_vals[n0:].any()) and not bool(s.node_msg_ts[n0:].any())
    assert s.nodes_with_messages == set(range(n0))                     # no new node holds one
    assert not bool(s.has_msg_mask()[n0:].any())
    p = s.has_msg_bits.data_ptr()
    cap = s._stores['node_msg_vals'].shape[0]
    assert s.grow(cap) is False and s.has_msg_bits.data_ptr() == p and s.has_msg_bits.numel() == hip_ops.bitmap_words(cap)
    assert s.grow(cap + 1) is True
    with pytest.raises(ValueError, match='never released'):
        s.grow(n0)
    big = MessageStoreNoGradLastOnly(cap + 1, 6)                       # (non-persistent buffers: compared directly)
    assert big.has_msg_bits.shape == s.has_msg_bits.shape and big.node_msg_vals.shape == s.node_msg_vals.shape


def test_append_node_rows():
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    rs = np.random.RandomState(0)
    rows = torch.from_numpy(rs.standard_normal((80, 8)).astype(np.float32))
    fg = NumericalFeature(torch.zeros(10, 8), None, dim=8)
    assert fg.nfeats_all_zero()
    assert fg.append_node_rows(3) is True and fg.n_nodes == 13 and fg.nfeats_all_zero()      # an int: zero rows
    p = fg.nfeats.data_ptr()
    assert fg.append_node_rows(rows[:5]) is False and fg.nfeats.data_ptr() == p and fg.n_nodes == 18
    assert not fg.nfeats_all_zero()                                                          # notices the appended rows
    assert torch.equal(fg.nfeats[13:], rows[:5]) and not bool(fg.nfeats[:13].any())
    assert fg.append_node_rows(rows[5:60]) is True and fg.nfeats.shape == (73, 8) and fg._version_ == 3
    assert torch.equal(fg.nfeats[13:], rows[:60])
    assert fg.append_node_rows(0) is False and fg.n_nodes == 73
    assert fg.append_node_rows(1, reserve=74) is True and fg._stores['nfeats'].shape[0] == 74      # reserve=: rows of the new store
    assert fg.append_node_rows(1, reserve=75) is True and fg._stores['nfeats'].shape[0] == 75 and fg.n_nodes == 75
    with pytest.raises(ValueError, match='reserve'):
        fg.append_node_rows(2, reserve=76)
    assert fg.n_nodes == 75 and torch.equal(fg.nfeats[13:73], rows[:60]) and not bool(fg.nfeats[73:].any())
    with pytest.raises(ValueError, match='width'):
        fg.append_node_rows(rows[:2, :7])
    with pytest.raises(ValueError):
        fg.append_node_rows(-1)
    with pytest.raises(NotImplementedError, match='no node table'):
        NumericalFeature(None, rows[:10], dim=8).append_node_rows(2)
    pinned = NumericalFeature(rows[:10], None, dim=8, register_buffer=False)
    with pytest.raises(NotImplementedError, match='pinned'):
        pinned.append_node_rows(2)
    assert fg.n_nodes == 75 and pinned.n_nodes == 10


def test_bitmap_grown():
    from www2023tiger_amd import hip_ops
    b = torch.tensor([5, -1], dtype=torch.int64)
    assert hip_ops.bitmap_grown(b, 128) is b
    g = hip_ops.bitmap_grown(b, 129)
    assert g.tolist() == [5, -1, 0]
    with pytest.raises(ValueError, match='bitmap_grown'):
        hip_ops.bitmap_grown(b, 64)
    with pytest.raises(ValueError, match='bitmap_grown'):
        hip_ops.bitmap_grown(b.int(), 200)
