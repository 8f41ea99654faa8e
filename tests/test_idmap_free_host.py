"""Removing keys and recycling dense ids without a GPU: the host twins (tg_idmap_remove_host / _assign_recycle_host /
_rebuild_free_host) and IdMap('cpu') against the reference loop (tests/_idmap_free_ref.py: a dict, a heap, a set) - ids, the
ids given out, the released ids, size, key_of and the bitmap bit for bit; the table as a set of (key, id) pairs.  The cases
are those of tests/_idmap_free_cases.py, which tests/test_hip_idmap_free.py runs through the kernels."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import _idmap_free_cases as cases
from _idmap_free_ref import INT32_MAX, RefFreeMap, fresh_keys, host_assign_recycle, host_remove, np_bits
from _idmap_ref import INT64_MIN, host_assign, host_lookup, keys_at_home, np_struct, np_tables
from www2023tiger_amd import _lib, hip_ops
from www2023tiger_amd._lib import TG_EINVAL, lib, ptr
from www2023tiger_amd.data.idmap import IdMap

CPU = ('cpu',)


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))


def test_symbols_and_workspaces():
    assert lib.tg_abi_version() == 9                       # entries are added; nothing that exists changed
    for name in ('tg_idmap_remove', 'tg_idmap_assign_recycle', 'tg_idmap_rebuild_free', 'tg_idmap_remove_host',
                 'tg_idmap_assign_recycle_host', 'tg_idmap_rebuild_free_host'):
        assert getattr(lib, name) is not None
    a16 = lambda x: (x + 15) // 16 * 16
    for n in (0, 1, 256, 257, 2049):
        assert lib.tg_idmap_remove_workspace_bytes(n) == a16(4 * n)
        for size, tiles in ((1, 1), (131072, 1), (131073, 2), (140000, 2), (3 * 131072 + 1, 4)):
            want = lib.tg_idmap_assign_workspace_bytes(n) + a16(4 * tiles) + 16
            assert lib.tg_idmap_assign_recycle_workspace_bytes(n, size) == want, (n, size)
    assert lib.tg_idmap_remove_workspace_bytes(-1) == 0 and lib.tg_idmap_assign_recycle_workspace_bytes(4, 0) == 0


@pytest.mark.parametrize('n', cases.SIZES)
def test_assign_and_remove_against_the_reference(n):
    cases.case_sizes(CPU, n)


def test_free_ids_on_both_sides_of_a_word_edge():
    cases.case_word_edge(CPU)


def test_free_ids_on_both_sides_of_a_select_tile_edge():
    cases.case_tile_edge(CPU)


def test_remove_duplicates_unknown_keys_the_padding_key_and_keys_that_come_back():
    cases.case_remove_forms(CPU)


def test_a_chain_that_wraps_stays_intact_when_its_middle_is_removed():
    cases.case_wrapping_chain(CPU, keys_at_home)


def test_batch_cut_invariance_between_removes():
    cases.case_cut_invariance(CPU)


def test_heavy_duplicates():
    cases.case_heavy_duplicates(CPU)


def test_churn_keeps_size_and_capacity_bounded():
    """64 live keys; 200 rounds remove 16 and assign 16 never-seen ones.  Without recycling the ids reach 3265 and the table
    8192 slots; with it size can never pass 64 live + the padding id + 16 free = 81 (here every round refills the pool it
    drained: 65) and the table stays at 256 slots, purged of the removed keys' slots whenever the used ones would pass half
    of it."""
    (m,), ref = cases.make(CPU)
    live = fresh_keys(64, 1 << 32)
    cases.assign([m], ref, live, 'the first 64')
    rs = np.random.RandomState(2)
    for r in range(200):
        out = rs.permutation(64)[:16]
        cases.remove([m], ref, live[out], f'round {r}')
        new = fresh_keys(16, (r + 2) << 32)
        ids = cases.assign([m], ref, new, f'round {r}')
        assert sorted(ids.tolist()) == sorted(ref.lookup(new).tolist()) and ref.n_free == 0
        live[out] = new
        assert m.size <= 81 and m.capacity <= 512, (r, m.size, m.capacity)
        assert torch.equal(m.lookup(tt(live)), torch.from_numpy(ref.lookup(live))) and bool((m.lookup(tt(live)) > 0).all())
    assert ref.capacity == 256 and m.capacity == 256 and m.size == 65


def test_a_map_that_never_removes_grows_as_before():
    m, ref = IdMap('cpu', capacity=16, reserve=8), RefFreeMap(16)
    caps = []
    for b in range(5):
        keys = (1000 * (b + 1) + np.arange(7)).astype(np.int64) * 104729
        cases.assign([m], ref, keys, f'batch {b}')
        caps.append(m.capacity)
    assert caps == [16, 32, 64, 64, 128] and m.size == 36 and m.n_free == 0 and m.slots_used == 36


def through_a_file(sd):
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    return torch.load(f, weights_only=True)


def holed():
    m, ref = IdMap('cpu', capacity=16), RefFreeMap(16)
    keys = fresh_keys(200, 1 << 32)
    cases.assign([m], ref, keys)
    cases.remove([m], ref, keys[[2, 62, 63, 64, 130, 198]])
    return m, ref, keys


def test_state_round_trip_with_and_without_holes():
    m, ref, keys = holed()
    sd = through_a_file(m.state_dict())
    assert sd['format'] == 'tiger-idmap-free' and sd['version'] == 1 and sd['key_of'].shape == (201,)
    assert sd['free'].dtype == torch.int64 and sd['free'].tolist() == [3, 63, 64, 65, 131, 199]
    assert (sd['key_of'][sd['free']] == INT64_MIN).all() and int((sd['key_of'] == INT64_MIN).sum()) == 7
    back = IdMap.from_state_dict(sd, 'cpu')
    assert (back.size, back.n_free) == (m.size, m.n_free) and torch.equal(back.key_of[:back.size], m.key_of[:m.size])
    assert back.free_ids().tolist() == m.free_ids().tolist()
    assert cases.live_pairs(back.slot_key.numpy(), back.slot_id.numpy()) == ref.pairs()
    more = [np.concatenate([fresh_keys(4, 5 << 32), keys[[2, 7]], [INT64_MIN]]), fresh_keys(300, 6 << 32)[::-1].copy()]
    for batch in more:                                   # the loaded map assigns exactly as the saved one
        want = ref.assign(batch)
        assert torch.equal(back.assign(tt(batch)), m.assign(tt(batch))) and np.array_equal(m.assign(tt(batch)).numpy(), want)
        assert back.size == m.size == ref.size and torch.equal(back.key_of[:back.size], m.key_of[:m.size])
    # the holes are filled: the map saves the version-1 dict of a map that never removed, and loads from it
    assert m.n_free == 0
    sd = through_a_file(m.state_dict())
    assert sorted(sd) == ['format', 'key_of', 'version'] and sd['format'] == 'tiger-idmap' and sd['version'] == 1
    back = IdMap.from_state_dict(sd, 'cpu')
    assert torch.equal(back.key_of[:back.size], m.key_of[:m.size]) and back.n_free == 0


def test_states_whose_free_list_is_no_free_list_are_refused_with_the_row():
    m, _, keys = holed()
    sd = m.state_dict()

    def bad(free=None, format=None, version=None, **rows):
        out = dict(sd, key_of=sd['key_of'].clone(), free=sd['free'].clone() if free is None else free)
        for row, value in rows.items():
            out['key_of'][int(row[1:])] = value
        if format:
            out['format'] = format
        if version:
            out['version'] = version
        return out

    f = sd['free']
    table = [(bad(free=f[[0, 2, 1, 3, 4, 5]]), r'ascend.*entry 2\b'), (bad(free=f[[0, 1, 1, 3, 4, 5]]), r'ascend.*entry 2\b'),
             (bad(free=torch.cat([torch.tensor([0]), f])), r'outside \[1, 201\)'),
             (bad(free=torch.cat([f, torch.tensor([201])])), r'outside \[1, 201\)'),
             (bad(free=f.int()), 'free must be'), (bad(free=f[:0]), 'free must be'), (bad(free=f.tolist()), 'free must be'),
             (bad(free=f[1:]), r'EMPTY_KEY.*row 3\b'),                                    # a hole that is not listed
             (bad(r130=INT64_MIN), r'EMPTY_KEY.*row 130\b'),
             (bad(free=torch.tensor([3, 63, 64, 65, 100, 131, 199])), r'FREE.*row 100\b'),    # listed, but it holds a key
             (bad(r63=12345), r'FREE.*row 63\b'),
             (bad(r63=12345, r20=INT64_MIN), r'EMPTY_KEY.*row 20\b'),                     # the smallest offending row
             (bad(r150=int(sd['key_of'][7])), r'DUP.*row 150\b'),
             (bad(version=2), 'version 2'), (bad(format='tiger-graph'), 'not a saved id map'), (bad(r0=5), 'padding')]
    for case, pattern in table:
        with pytest.raises(ValueError, match=pattern):
            IdMap.from_state_dict(case, 'cpu')
    # what the version-1 format refuses stays refused: another version, INT64_MIN in a row, a free list it does not know
    v1 = {'format': 'tiger-idmap', 'version': 1, 'key_of': sd['key_of'].clone()}
    with pytest.raises(ValueError, match=r'EMPTY_KEY.*row 3\b'):
        IdMap.from_state_dict(v1, 'cpu')
    with pytest.raises(ValueError, match='version 2'):
        IdMap.from_state_dict(dict(v1, version=2), 'cpu')


def test_the_c_entries_refuse_before_they_touch_anything():
    keys = np.arange(1, 9, dtype=np.int64)

    def seeded(capacity=64, key_rows=64):
        t = np_tables(capacity, key_rows)
        assert host_assign(t, 1, np.arange(101, 111))[2] == (11, 0)      # ids 1 .. 10
        bits = np_bits(key_rows)
        rc, ids, rel, out2 = host_remove(t, 11, bits, np.array([103, 104]))
        assert rc == 0 and ids.tolist() == [3, 4] and rel.tolist() == [3, 4] and out2 == (2, 0) and bits[0] == 0b11000
        return t, bits

    t, bits = seeded()
    refused = [('2 (occupied + n) > capacity', dict(occupied=25)), ('size + (n - n_free) > key_rows', dict(size=59, n_free=2)),
               ('n_free >= size', dict(n_free=11)), ('n_free < 0', dict(n_free=-1)), ('size 0', dict(size=0)),
               ('occupied < 0', dict(occupied=-1)), ('a bitmap shorter than size', dict(words=0)),
               ('capacity 48', dict(capacity=48)), ('capacity 8', dict(capacity=8))]
    for label, kw in refused:
        before = [a.copy() for a in t] + [bits.copy()]
        args = dict(size=11, occupied=11, n_free=2, capacity=None, words=None)
        args.update(kw)
        rc, ids, fl, out2 = host_assign_recycle(t, args['size'], args['occupied'], bits, args['n_free'], keys,
                                                capacity=args['capacity'], words=args['words'])
        assert rc == TG_EINVAL, label
        assert (ids == -7).all() and (fl == -7).all() and out2 == (-7, -7), label
        assert all(np.array_equal(a, b) for a, b in zip(t + (bits,), before)), label
    m = np_struct(t)
    ids, rel, out2, fl = (np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32), np.zeros(2, dtype=np.int64),
                          np.zeros(8, dtype=np.int32))
    assert lib.tg_idmap_assign_recycle_host(C.byref(m), 11, 11, None, 1, 2, ptr(keys), 8, ptr(ids), ptr(fl), ptr(out2)) == TG_EINVAL
    assert lib.tg_idmap_assign_recycle_host(C.byref(m), 11, 11, ptr(bits), 1, 2, ptr(keys), 8, ptr(ids), None, ptr(out2)) == TG_EINVAL
    assert lib.tg_idmap_assign_recycle_host(C.byref(m), 11, 11, ptr(bits), 1, 2, ptr(keys), 8, ptr(ids), ptr(fl), None) == TG_EINVAL
    assert lib.tg_idmap_remove_host(C.byref(m), 11, None, 1, ptr(keys), 8, ptr(ids), ptr(rel), ptr(out2)) == TG_EINVAL
    assert lib.tg_idmap_remove_host(C.byref(m), 65, ptr(bits), 1, ptr(keys), 8, ptr(ids), ptr(rel), ptr(out2)) == TG_EINVAL
    assert lib.tg_idmap_remove_host(C.byref(m), 11, ptr(bits), 1, ptr(keys), -1, ptr(ids), ptr(rel), ptr(out2)) == TG_EINVAL
    assert lib.tg_idmap_remove_host(C.byref(m), 11, ptr(bits), 1, ptr(keys), 8, ptr(ids), None, ptr(out2)) == TG_EINVAL
    assert lib.tg_idmap_rebuild_free_host(C.byref(m), 11, 40, ptr(bits), 1, ptr(out2)) == TG_EINVAL      # 2 live > capacity
    assert lib.tg_idmap_rebuild_free_host(C.byref(m), 11, 0, ptr(bits), 1, ptr(out2)) == TG_EINVAL
    # the device entries make the same checks before any launch: no GPU is needed to be refused
    ws = np.zeros(1 << 12, dtype=np.uint8)
    assert lib.tg_idmap_assign_recycle(C.byref(m), 11, 25, ptr(bits), 1, 2, ptr(keys), 8, ptr(ids), ptr(fl), ptr(out2), ptr(ws),
                                       ws.nbytes, None) == TG_EINVAL
    assert lib.tg_idmap_assign_recycle(C.byref(m), 59, 11, ptr(bits), 1, 2, ptr(keys), 8, ptr(ids), ptr(fl), ptr(out2), ptr(ws),
                                       ws.nbytes, None) == TG_EINVAL
    assert lib.tg_idmap_assign_recycle(C.byref(m), 11, 11, ptr(bits), 1, 2, ptr(keys), 8, ptr(ids), ptr(fl), ptr(out2), ptr(ws),
                                       8, None) == _lib.TG_EWORKSPACE
    assert lib.tg_idmap_remove(C.byref(m), 65, ptr(bits), 1, ptr(keys), 8, ptr(ids), ptr(rel), ptr(out2), ptr(ws), ws.nbytes,
                               None) == TG_EINVAL
    assert lib.tg_idmap_remove(C.byref(m), 11, ptr(bits), 1, ptr(keys), 8, ptr(ids), ptr(rel), ptr(out2), ptr(ws), 8,
                               None) == _lib.TG_EWORKSPACE
    assert lib.tg_idmap_rebuild_free(C.byref(m), 11, 40, ptr(bits), 1, ptr(out2), None) == TG_EINVAL
    # a well-formed call on the same arrays goes through: ids 3 and 4 first, then the tail
    rc, ids, fl, out2 = host_assign_recycle(t, 11, 11, bits, 2, np.array([7, 105, 8, INT64_MIN, 9, 7]))
    assert rc == 0 and ids.tolist() == [3, 5, 4, 0, 11, 3] and fl.tolist() == [3, 4] and out2 == (14, 0) and bits[0] == 0
    assert host_lookup(t, np.array([103, 7, 8, 9])).tolist() == [-1, 3, 4, 11]


def test_a_bitmap_that_disagrees_with_n_free_is_reported_not_followed():
    t = np_tables(64, 64)
    host_assign(t, 1, np.arange(101, 111))
    bits = np_bits(64)
    host_remove(t, 11, bits, np.array([103, 104]))
    rc, ids, fl, out2 = host_assign_recycle(t, 11, 11, bits, 3, np.array([7, 8, 9, 10]))     # three are claimed free, two are
    assert rc == 0 and out2[1] & _lib.TG_IDMAP_ERR_FREE and ids.tolist()[:2] == [3, 4] and ids[2] == -1
    assert 'FREE' in hip_ops.IDMAP_ERR_TEXT(_lib.TG_IDMAP_ERR_FREE)
    word = ((0x7FFFFFFF - 12) << 8) | _lib.TG_IDMAP_ERR_FREE
    assert 'row 12 ' in hip_ops.IDMAP_ERR_TEXT(word)


def test_the_wrapper_refuses_and_documents():
    m, _, keys = holed()
    for bad in (torch.tensor([1, 2], dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), [1, 2]):
        with pytest.raises(ValueError, match='contiguous 1-d int64'):
            m.remove(bad)
    with pytest.raises(ValueError, match='outside'):
        m.is_free(torch.tensor([m.size]))
    with pytest.raises(ValueError, match='int32 or int64'):
        m.is_free(torch.tensor([1.0]))
    assert m.is_free(torch.tensor([[0, 3], [4, 63]], dtype=torch.int32)).tolist() == [[False, True], [False, True]]
    assert m.size == 201 and m.n_free == 6 and INT32_MAX not in m.remove(tt(keys[:5]))[1].tolist()
