"""The cases the host and the device tests of key removal share (tests/test_idmap_free_host.py: IdMap('cpu') alone;
tests/test_hip_idmap_free.py: the device map AND the host twin).  Every case drives a list of maps and the reference
(_idmap_free_ref.RefFreeMap) with the same calls and compares after each: ids, the ids given out, the released ids, size,
n_free, key_of, the bitmap, the capacity and - as a set of (key, id) pairs - the table."""
import numpy as np
import torch

from _idmap_free_ref import RefFreeMap, bits_to_ids, fresh_keys, live_pairs
from _idmap_ref import INT64_MIN
from www2023tiger_amd.data.idmap import IdMap

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)   # 256 / 257: the one-workgroup forms' limit
FREE_MODES = (0, 1, 63, 64, 65, 'below', 'equal', 'above')


def tt(a, device):
    return torch.from_numpy(np.array(a, dtype=np.int64)).to(device)


def make(devices, capacity=16, reserve=None):
    return [IdMap(d, capacity=capacity, reserve=reserve) for d in devices], RefFreeMap(capacity)


def same(maps, ref, what=''):
    want_key_of, want_free, want_pairs = torch.from_numpy(ref.key_of()), sorted(ref.free), ref.pairs()
    for m in maps:
        tag = f'{what} [{m.device}]'
        assert (m.size, m.n_free, m.capacity, m.slots_used) == (ref.size, ref.n_free, ref.capacity, ref.slots_used), tag
        assert torch.equal(m.key_of[:m.size].cpu(), want_key_of), tag
        assert bool((m.key_of[m.size:] == INT64_MIN).all()), tag
        assert bits_to_ids(m.free_bits.cpu().numpy(), m.size).tolist() == want_free, tag
        assert m.free_ids().tolist() == want_free, tag
        assert live_pairs(m.slot_key.cpu().numpy(), m.slot_id.cpu().numpy()) == want_pairs, tag


def assign(maps, ref, keys, what=''):
    want, want_new = ref.assign(keys, return_new=True)
    for m in maps:
        ids, new = m.assign(tt(keys, m.device), return_new=True)
        assert ids.dtype == torch.int32 and new.dtype == torch.int32 and ids.device == m.device, what
        assert torch.equal(ids.cpu(), torch.from_numpy(want)), f'{what} [{m.device}]'
        assert torch.equal(new.cpu(), torch.from_numpy(want_new)), f'{what} [{m.device}] (the ids given out)'
    same(maps, ref, what)
    return want


def remove(maps, ref, keys, what=''):
    want, want_gone = ref.remove(keys)
    for m in maps:
        ids, gone = m.remove(tt(keys, m.device))
        assert ids.dtype == torch.int32 and gone.dtype == torch.int32, what
        assert torch.equal(ids.cpu(), torch.from_numpy(want)), f'{what} [{m.device}]'
        assert torch.equal(gone.cpu(), torch.from_numpy(want_gone)), f'{what} [{m.device}] (the released ids)'
    same(maps, ref, what)
    return want, want_gone


def lookups(maps, ref, keys, what=''):
    want = torch.from_numpy(ref.lookup(keys))
    for m in maps:
        assert torch.equal(m.lookup(tt(keys, m.device)).cpu(), want), f'{what} [{m.device}]'


def batch_for(n, mode, seed=0):
    """-> base keys, the keys to remove first, the batch of n, for one batch size and one free-pool mode.  The batch mixes
    never-seen keys (with repeats), live keys, the padding key and - in the numeric modes - removed keys that come back."""
    rs = np.random.RandomState(1000 * seed + n)
    pool = fresh_keys(max(1, n // 2), 2 << 32)
    kind = rs.rand(n)
    pick = rs.randint(0, len(pool), size=n)
    n_fresh = len(set(pick[kind < 0.5].tolist()))
    n_free = {'below': max(n_fresh - 1, 0), 'equal': n_fresh, 'above': n_fresh + 7}.get(mode, mode)
    base = fresh_keys(n_free + 50, 1 << 32)
    gone = base[rs.permutation(len(base))[:n_free]]
    live = np.setdiff1d(base, gone)
    batch = np.where(kind < 0.5, pool[pick], live[rs.randint(0, len(live), size=n)])
    batch[kind > 0.9] = INT64_MIN
    if isinstance(mode, int) and n_free:
        back = (kind > 0.75) & (kind <= 0.9)
        batch[back] = gone[rs.randint(0, len(gone), size=n)][back]
    return base, gone, np.ascontiguousarray(batch, dtype=np.int64)


def case_sizes(devices, n):
    for mode in FREE_MODES:
        what = f'n = {n}, free = {mode}'
        base, gone, batch = batch_for(n, mode)
        maps, ref = make(devices)
        assign(maps, ref, base, what + ' (base)')
        remove(maps, ref, gone, what + ' (remove)')
        assert ref.n_free == len(gone)
        assign(maps, ref, batch, what)
        lookups(maps, ref, np.concatenate([batch, base]), what)
        assign(maps, ref, batch, what + ' (again: every key is known)')
        remove(maps, ref, batch, what + ' (the batch removed: duplicates, the padding key)')
        lookups(maps, ref, np.concatenate([batch, base]), what + ' (after the removal)')


def case_word_edge(devices):
    base = fresh_keys(130, 1 << 32)                      # ids 1 .. 130
    for ids in ([63], [64], [65], [63, 64, 65], [1, 63, 64, 65, 127, 128, 129]):
        maps, ref = make(devices)
        assign(maps, ref, base)
        _, gone = remove(maps, ref, base[np.array(ids) - 1], f'{ids}')
        assert gone.tolist() == ids
        for m in maps:
            assert m.is_free(torch.arange(131, device=m.device)).nonzero().flatten().tolist() == ids
            assert m.keys_of(torch.tensor(ids, device=m.device)).tolist() == [INT64_MIN] * len(ids)
        new = fresh_keys(len(ids) + 2, 3 << 32)
        got = np.concatenate([assign(maps, ref, new[:2], f'{ids} a'), assign(maps, ref, new[2:], f'{ids} b')])
        assert got.tolist() == ids + [131, 132]


def case_tile_edge(devices):
    """free ids on both sides of the select's tile edge (2048 words = 131 072 ids) on a map of 140 000 ids"""
    base = np.arange(1, 140000, dtype=np.int64) * 7 + (1 << 36)     # key of id i: 7 i + 2^36
    key = lambda ids: np.array(ids, dtype=np.int64) * 7 + (1 << 36)
    for ids, n in (([5, 131071, 131072, 131073, 139999], 3), ([131071, 131073], 1)):
        maps, ref = make(devices, capacity=1 << 19, reserve=140100)
        assign(maps, ref, base)
        assert ref.size == 140000
        _, gone = remove(maps, ref, key(ids)[::-1], f'{ids}')
        assert gone.tolist() == ids
        new = fresh_keys(len(ids) + 2, 3 << 32)
        got = np.concatenate([assign(maps, ref, new[:n], f'{ids} a'), assign(maps, ref, new[n:], f'{ids} b')])
        assert got.tolist() == ids + [140000, 140001]
        for m in maps:
            assert not bool(m.is_free(torch.tensor(ids, device=m.device)).any())


def case_remove_forms(devices):
    maps, ref = make(devices)
    base = fresh_keys(40, 1 << 32)
    assign(maps, ref, base)
    batch = np.array([base[3], 77, base[3], INT64_MIN, base[9], base[3], 78, base[0], INT64_MIN, base[9]], dtype=np.int64)
    ids, gone = remove(maps, ref, batch, 'duplicates, unknown keys, the padding key')
    assert ids.tolist() == [4, -1, 4, 0, 10, 4, -1, 1, 0, 10] and gone.tolist() == [1, 4, 10]
    ids, gone = remove(maps, ref, batch, 'removed twice, in two calls')
    assert ids.tolist() == [-1, -1, -1, 0, -1, -1, -1, -1, 0, -1] and gone.tolist() == []
    remove(maps, ref, np.zeros(0, dtype=np.int64), 'no key')
    remove(maps, ref, np.array([INT64_MIN], dtype=np.int64), 'the padding key alone')
    for m in maps:
        assert m.keys_of(torch.tensor([0, 1, 2, 4], device=m.device)).tolist() == [INT64_MIN, INT64_MIN, int(base[1]), INT64_MIN]
    # a removed key comes back: alone, then repeated inside a batch - a new key each time, the smallest free id first
    assert assign(maps, ref, base[9:10], 'back alone').tolist() == [1]
    assert assign(maps, ref, np.array([base[3], 5, base[3], base[0], base[3], base[0]], dtype=np.int64), 'back, repeated').tolist() \
        == [4, 10, 4, 41, 4, 41]
    lookups(maps, ref, np.concatenate([base, batch]))


def case_wrapping_chain(devices, keys_at_home):
    """20 keys with home slot 63 of 64: the chain is slot 63, then 0 .. 18.  The middle ones are removed: their slots keep
    their keys, so the later ones are still found, and a removed key that comes back takes its old slot - no second one."""
    keys = keys_at_home(63, 64, 20)
    maps, ref = make(devices, capacity=64)
    assign(maps, ref, keys[:10])
    assign(maps, ref, keys[10:])
    chain = list(range(19)) + [63]
    remove(maps, ref, keys[5:15], 'the middle of the chain')
    lookups(maps, ref, keys, 'behind the removed slots')
    for m in maps:
        assert m.capacity == 64 and torch.nonzero(m.slot_key != INT64_MIN).flatten().tolist() == chain
        assert m.lookup(tt(keys[15:], m.device)).tolist() == list(range(16, 21))
        assert m.lookup(tt(keys_at_home(63, 64, 25)[20:], m.device)).tolist() == [-1] * 5    # the probe ends at slot 19
    assert assign(maps, ref, keys[14:4:-1], 'back, in another order').tolist() == list(range(6, 16))
    for m in maps:
        assert m.capacity == 64 and torch.nonzero(m.slot_key != INT64_MIN).flatten().tolist() == chain
    lookups(maps, ref, keys)


def case_cut_invariance(devices):
    """one stream of assigns with two removes inside it; the assigns between two removes are cut in three ways"""
    rs = np.random.RandomState(5)
    parts = [rs.randint(0, 400, size=700).astype(np.int64) * 2654435761 - 77 for _ in range(3)]
    parts[1][[5, 150]] = INT64_MIN
    drops = [np.unique(parts[0])[::3], np.unique(np.concatenate(parts[:2]))[1::4]]
    cuts = {'whole': [0, 700], 'by 1 and ragged': list(range(0, 40)) + [40, 100, 104, 105, 180, 300, 557, 700],
            'by 70': list(range(0, 701, 70))}
    results = []
    for name, c in cuts.items():
        maps, ref = make(devices)
        ids = []
        for p, part in enumerate(parts):
            ids += [assign(maps, ref, part[a:b], f'{name}, part {p}') for a, b in zip(c[:-1], c[1:])]
            if p < 2:
                remove(maps, ref, drops[p], f'{name}, remove {p}')
        results.append((np.concatenate(ids), ref.key_of(), sorted(ref.free)))
    for r in results[1:]:
        assert np.array_equal(r[0], results[0][0]) and np.array_equal(r[1], results[0][1]) and r[2] == results[0][2]
    assert results[0][2], 'the stream should leave free ids behind'


def case_heavy_duplicates(devices):
    """64 keys x 128 copies shuffled over 8192 positions: removed in one call, then assigned again behind a free pool"""
    rs = np.random.RandomState(11)
    distinct = (1 << 41) + rs.permutation(1 << 16)[:64].astype(np.int64) * 1000003
    batch = rs.permutation(np.repeat(distinct, 128))
    base = fresh_keys(100, 1 << 32)
    maps, ref = make(devices)
    assign(maps, ref, base, 'base')
    assign(maps, ref, distinct[::-1].copy(), 'the 64 keys')
    _, gone = remove(maps, ref, batch, 'heavy duplicates removed')
    assert len(gone) == 64 and ref.n_free == 64
    remove(maps, ref, base[10:40], 'thirty more')
    ids = assign(maps, ref, batch, 'heavy duplicates assigned behind 94 free ids')
    assert ref.n_free == 30 and len(np.unique(ids)) == 64
    return [(m.key_of[:m.size].cpu(), m.free_ids()) for m in maps], ids
