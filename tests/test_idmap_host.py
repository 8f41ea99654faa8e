"""The id map without a GPU: the host twins (tg_idmap_*_host) and IdMap on the CPU against the Python loop the assignment
rule is defined by - ids, size and key_of bit for bit -, colliding keys whose chains wrap past the end of the table, growth,
batch-cut invariance, the state round trip and what the C entry and the wrapper refuse."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest
import torch

from _idmap_ref import (INT64_MAX, INT64_MIN, KNOWN, SIZES, RefMap, collision_batches, cut_stream, host_assign, host_lookup, keys_at_home,
                        mixes, np_struct, np_tables, pairs, ref_hash)
from www2023tiger_amd import _lib, hip_ops
from www2023tiger_amd._lib import TG_EINVAL, lib, ptr
from www2023tiger_amd.data.idmap import IdMap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))


def seeded():
    """a CPU map and its reference, both holding KNOWN"""
    m, ref = IdMap('cpu', capacity=16), RefMap()
    assert np.array_equal(m.assign(tt(KNOWN)).numpy(), ref.assign(KNOWN))
    return m, ref


def same_map(m, ref, what=''):
    assert m.size == ref.size, what
    np.testing.assert_array_equal(m.key_of[:m.size].numpy(), ref.key_of(), err_msg=what)
    assert bool((m.key_of[m.size:] == INT64_MIN).all()), what
    assert pairs(m.slot_key.numpy(), m.slot_id.numpy()) == {(k, v) for k, v in ref.d.items() if v}, what


def test_symbols_layout_and_hash(tmp_path):
    assert lib.tg_abi_version() == 9
    for name in ('tg_idmap_lookup', 'tg_idmap_assign', 'tg_idmap_rebuild', 'tg_idmap_assign_workspace_bytes',
                 'tg_idmap_lookup_host', 'tg_idmap_assign_host', 'tg_idmap_rebuild_host', 'tg_idmap_hash'):
        assert getattr(lib, name) is not None
    a16 = lambda x: (x + 15) // 16 * 16
    for n, tiles in ((0, 0), (1, 1), (2048, 1), (2049, 2), (4097, 3)):
        want = 2 * a16(4 * n) + a16(256 * tiles) + 2 * a16(4 * tiles) + a16(4 * (tiles + 1))
        assert lib.tg_idmap_assign_workspace_bytes(n) == want, n
    assert lib.tg_idmap_assign_workspace_bytes(-1) == 0
    for key in (0, 1, -1, INT64_MAX, INT64_MIN + 1, 123456789):
        assert lib.tg_idmap_hash(key) == ref_hash(key), key
    src = tmp_path / 'layout.c'
    fields = [f for f, _ in _lib.TgIdmap._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tiger_hip.h"\nint main(void) {\n'
                   '  printf("%zu %d %d\\n", sizeof(tg_idmap), TG_ABI_VERSION, TG_IDMAP_EMPTY == INT64_MIN);\n'
                   + ''.join(f'  printf("%zu\\n", offsetof(tg_idmap, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out[:3]] == [C.sizeof(_lib.TgIdmap), 9, 1]
    assert [int(x) for x in out[3:]] == [getattr(_lib.TgIdmap, f).offset for f in fields]


@pytest.mark.parametrize('n', SIZES)
def test_assign_against_the_reference(n):
    for name, keys in mixes(n, KNOWN).items():
        m, ref = seeded()
        before = m.size
        ids = m.assign(tt(keys))
        assert ids.dtype == torch.int32 and ids.shape == (n,)
        np.testing.assert_array_equal(ids.numpy(), ref.assign(keys), err_msg=name)
        same_map(m, ref, name)
        if name in ('all-known', 'padding-key'):
            assert m.size == before, name
        if name == 'one-new-key':
            assert m.size == before + (n > 0)
        if name in ('padding-key', 'padding-among-new'):
            assert bool((ids[tt(keys) == INT64_MIN] == 0).all()) and bool((ids[tt(keys) != INT64_MIN] > 0).all())
        # the same batch again: every key is known now, nothing changes
        np.testing.assert_array_equal(m.assign(tt(keys)).numpy(), ids.numpy())
        same_map(m, ref, name + ' (again)')


def test_edge_keys_are_ordinary_keys():
    m, ref = IdMap('cpu', capacity=16), RefMap()
    keys = np.array([0, -1, INT64_MAX, INT64_MIN + 1, INT64_MIN, 0, INT64_MIN + 1], dtype=np.int64)
    ids = m.assign(tt(keys))
    assert ids.tolist() == [1, 2, 3, 4, 0, 1, 4] == ref.assign(keys).tolist()
    assert m.size == 5 and m.keys_of(torch.tensor([0, 4, 3])).tolist() == [INT64_MIN, INT64_MIN + 1, INT64_MAX]
    same_map(m, ref)


def test_chains_that_wrap_past_the_end_of_the_table():
    cap = 64
    keys = keys_at_home(63, cap, 20)
    assert len(set(keys.tolist())) == 20 and all(ref_hash(int(k)) & (cap - 1) == 63 for k in keys)
    assert all(lib.tg_idmap_hash(int(k)) & (cap - 1) == 63 for k in keys)
    m, ref = IdMap('cpu', capacity=cap), RefMap()
    for batch in collision_batches(keys):
        np.testing.assert_array_equal(m.assign(tt(batch)).numpy(), ref.assign(batch))
    batch = np.concatenate(collision_batches(keys))
    assert m.capacity == cap                                        # 21 ids: not grown, so the chain is one run of slots
    same_map(m, ref)
    used = np.nonzero(m.slot_key.numpy() != INT64_MIN)[0]
    assert used.tolist() == list(range(19)) + [63]                  # slot 63, then 0 .. 18: the chain wrapped
    np.testing.assert_array_equal(m.lookup(tt(batch)).numpy(), ref.lookup(batch))
    other = keys_at_home(63, cap, 25)[20:]                          # same home, not in the map: the probe ends at slot 19
    assert m.lookup(tt(other)).tolist() == [-1] * 5


def test_growth_doubles_the_capacity_and_keeps_every_lookup():
    m, ref = IdMap('cpu', capacity=16, reserve=8), RefMap()
    caps, every = [], np.zeros(0, dtype=np.int64)
    for b in range(5):
        keys = (1000 * (b + 1) + np.arange(7)).astype(np.int64) * 104729
        np.testing.assert_array_equal(m.assign(tt(keys)).numpy(), ref.assign(keys))
        every = np.concatenate([every, keys])
        caps.append(m.capacity)
        np.testing.assert_array_equal(m.lookup(tt(every)).numpy(), ref.lookup(every))
        same_map(m, ref, f'batch {b}')
        assert m.key_of.numel() >= m.size
    assert caps == [16, 32, 64, 64, 128]
    assert m.size == 36


def test_batch_cut_invariance():
    stream, runs = cut_stream()
    want = RefMap()
    want_ids = want.assign(stream)
    for name, cuts in runs.items():
        m = IdMap('cpu', capacity=16)
        ids = np.concatenate([m.assign(tt(stream[a:b])).numpy() for a, b in zip(cuts[:-1], cuts[1:])])
        np.testing.assert_array_equal(ids, want_ids, err_msg=name)
        same_map(m, want, name)


def test_lookup_changes_nothing():
    m, ref = seeded()
    before = [t.clone() for t in m.tables]
    keys = np.concatenate([KNOWN, [INT64_MIN, 123, -123, INT64_MAX], KNOWN[::-1]]).astype(np.int64)
    ids = m.lookup(tt(keys))
    assert ids.dtype == torch.int32
    np.testing.assert_array_equal(ids.numpy(), ref.lookup(keys))
    assert ids[len(KNOWN)].item() == 0 and ids[len(KNOWN) + 1:len(KNOWN) + 4].tolist() == [-1, -1, -1]
    assert m.size == ref.size and all(torch.equal(a, b) for a, b in zip(m.tables, before))
    assert m.lookup(tt([])).shape == (0,)


def through_a_file(sd):
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    return torch.load(f, weights_only=True)


def test_from_keys_and_state_round_trip():
    keys = (np.arange(1, 200).astype(np.int64) * 0x9E3779B1) ^ 0x5555
    m = IdMap.from_keys(tt(keys), 'cpu')
    assert m.size == 200 and m.lookup(tt(keys)).tolist() == list(range(1, 200))
    assert m.keys_of(torch.arange(200, dtype=torch.int32))[1:].tolist() == keys.tolist()
    more = [np.array([7, keys[3], 8, 7, INT64_MIN, 9], dtype=np.int64), (np.arange(3000) % 1700 + (1 << 45)).astype(np.int64)]
    m.assign(tt(more[0]))
    sd = through_a_file(m.state_dict())
    assert sd['format'] == 'tiger-idmap' and sd['version'] == 1 and sd['key_of'].shape == (m.size,)
    back = IdMap.from_state_dict(sd, 'cpu')
    assert back.size == m.size and torch.equal(back.key_of[:back.size], m.key_of[:m.size])
    assert pairs(back.slot_key.numpy(), back.slot_id.numpy()) == pairs(m.slot_key.numpy(), m.slot_id.numpy())
    for batch in (more[1], more[0]):
        assert torch.equal(back.assign(tt(batch)), m.assign(tt(batch)))
        assert back.size == m.size and torch.equal(back.key_of[:back.size], m.key_of[:m.size])
    with pytest.raises(ValueError, match=r'outside \[0, '):
        m.keys_of(torch.tensor([m.size]))
    with pytest.raises(ValueError, match='outside'):
        m.keys_of(torch.tensor([-1]))


def test_states_that_are_no_mapping_are_refused_with_the_row():
    m = IdMap.from_keys(tt(np.arange(10, 30)), 'cpu')
    sd = m.state_dict()

    def bad(**kw):
        out = dict(sd, key_of=sd['key_of'].clone())
        for k, v in kw.items():
            if isinstance(v, tuple):
                out[k][v[0]] = v[1]
            else:
                out[k] = v
        return out

    cases = [(bad(key_of=(7, int(sd['key_of'][2]))), r'DUP.*row 7\b'), (bad(key_of=(3, INT64_MIN)), r'EMPTY_KEY.*row 3\b'),
             (bad(key_of=(0, 5)), 'padding'), (bad(format='tiger-graph'), 'not a saved id map'), (bad(version=2), 'version 2'),
             (bad(key_of=sd['key_of'].int()), 'int64'), (bad(key_of=sd['key_of'][:0]), 'padding row')]
    for case, pattern in cases:
        with pytest.raises(ValueError, match=pattern):
            IdMap.from_state_dict(case, 'cpu')
    both = bad(key_of=(9, int(sd['key_of'][1])))
    both['key_of'][4] = INT64_MIN
    with pytest.raises(ValueError, match=r'EMPTY_KEY.*row 4\b'):    # the smallest offending row
        IdMap.from_state_dict(both, 'cpu')
    with pytest.raises(ValueError, match=r'DUP.*row 3\b'):
        IdMap.from_keys(tt([4, 5, 4, 5]), 'cpu')
    with pytest.raises(ValueError, match=r'EMPTY_KEY.*row 2\b'):
        IdMap.from_keys(tt([4, INT64_MIN]), 'cpu')


def test_the_c_entry_refuses_before_it_touches_anything():
    keys = np.arange(1, 9, dtype=np.int64)
    t = np_tables(64, 64)
    t48 = np_tables(48, 64)
    for label, tables, cap, size, k in [('capacity 48', t48, None, 1, keys), ('capacity 8', t, 8, 1, keys[:1]),
                                        ('2 (size + n) > capacity', np_tables(16, 64), None, 1, keys),
                                        ('key_of too short', np_tables(64, 8), None, 1, keys),
                                        ('size 0', t, None, 0, keys)]:
        before = [a.copy() for a in tables]
        rc, ids, out2 = host_assign(tables, size, k, capacity=cap)
        assert rc == TG_EINVAL, label
        assert (ids == -7).all() and out2 == (-7, -7), label
        assert all(np.array_equal(a, b) for a, b in zip(tables, before)), label
    m = np_struct(t)
    ids, out2 = np.zeros(8, dtype=np.int32), np.zeros(2, dtype=np.int64)
    assert lib.tg_idmap_assign_host(C.byref(m), 1, ptr(keys), -1, ptr(ids), ptr(out2)) == TG_EINVAL
    assert lib.tg_idmap_assign_host(C.byref(m), 1, ptr(keys), 8, ptr(ids), None) == TG_EINVAL
    # the device entries make the same checks before any launch: no GPU is needed to be refused
    m48 = np_struct(t48)
    assert lib.tg_idmap_assign(C.byref(m48), 1, ptr(keys), 8, ptr(ids), ptr(out2), ptr(out2), 1 << 20, None) == TG_EINVAL
    assert lib.tg_idmap_lookup(C.byref(m48), ptr(keys), 8, ptr(ids), None) == TG_EINVAL
    assert lib.tg_idmap_rebuild(C.byref(m48), 1, ptr(out2), None) == TG_EINVAL
    short = np_struct(np_tables(16, 64))
    assert lib.tg_idmap_assign(C.byref(short), 1, ptr(keys), 8, ptr(ids), ptr(out2), ptr(out2), 1 << 20, None) == TG_EINVAL
    assert lib.tg_idmap_assign(C.byref(m), 1, ptr(keys), 8, ptr(ids), ptr(out2), ptr(out2), 8, None) == _lib.TG_EWORKSPACE
    # a well-formed call on the same arrays goes through
    rc, ids, out2 = host_assign(t, 1, keys)
    assert rc == 0 and ids.tolist() == list(range(1, 9)) and out2 == (9, 0)
    assert host_lookup(t, np.array([3, 99, INT64_MIN])).tolist() == [3, -1, 0]


def test_the_wrapper_refuses_keys_that_are_no_int64_vector():
    m, _ = seeded()
    for keys in (torch.tensor([1, 2], dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64),
                 torch.arange(10, dtype=torch.int64)[::2], [1, 2], np.arange(3)):
        for fn in (m.assign, m.lookup):
            with pytest.raises(ValueError, match='contiguous 1-d int64'):
                fn(keys)
    assert m.size == len(KNOWN) + 1
    m.size = 0x7FFFFFFF - 1
    with pytest.raises(ValueError, match='2\\^31 - 1'):
        m.assign(tt([1, 2]))
    with pytest.raises(ValueError, match='power of two'):
        IdMap('cpu', capacity=48)


def test_error_text_names_class_and_row():
    word = ((0x7FFFFFFF - 12) << 8) | _lib.TG_IDMAP_ERR_DUP
    assert 'DUP' in hip_ops.IDMAP_ERR_TEXT(word) and 'row 12 ' in hip_ops.IDMAP_ERR_TEXT(word)
    assert 'PROBE' in hip_ops.IDMAP_ERR_TEXT(_lib.TG_IDMAP_ERR_PROBE) and 'row' not in hip_ops.IDMAP_ERR_TEXT(1)
