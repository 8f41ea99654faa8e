"""The id map kernels (tg_idmap_lookup / _assign / _rebuild) on the GPU: the cases of tests/test_idmap_host.py through the
device path, compared with the Python loop the rule is defined by AND with the host twin - ids, size and key_of with
torch.equal; the table only as a set of (key, id) pairs, since where a key sits may depend on the race for a slot.
n = 65 crosses a wavefront, 256 / 257 the one-workgroup form's limit, 2048 / 2049 a tile, 4097 the scan over tile counts.
No test fills a table or aims at the probe bound."""
import numpy as np
import pytest
import torch

from _idmap_ref import INT64_MIN, KNOWN, SIZES, RefMap, collision_batches, cut_stream, keys_at_home, mixes, pairs
from www2023tiger_amd.data.idmap import IdMap

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


def tt(a, device=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device or dev())


def table_pairs(m):
    return pairs(m.slot_key.cpu().numpy(), m.slot_id.cpu().numpy())


def same_map(g, h, ref, what=''):
    """device map g, host-twin map h, reference"""
    assert g.size == h.size == ref.size, what
    assert torch.equal(g.key_of[:g.size].cpu(), h.key_of[:h.size]), what
    assert torch.equal(h.key_of[:h.size], torch.from_numpy(ref.key_of())), what
    assert bool((g.key_of[g.size:] == INT64_MIN).all()), what
    assert table_pairs(g) == pairs(h.slot_key.numpy(), h.slot_id.numpy()) == {(k, v) for k, v in ref.d.items() if v}, what


def three(capacity=16):
    return IdMap(dev(), capacity=capacity), IdMap('cpu', capacity=capacity), RefMap()


def assign3(g, h, ref, keys, what=''):
    ids = g.assign(tt(keys))
    assert ids.dtype == torch.int32 and ids.device == dev()
    want = torch.from_numpy(ref.assign(keys))
    assert torch.equal(ids.cpu(), want), what
    assert torch.equal(h.assign(tt(keys, 'cpu')), want), what
    same_map(g, h, ref, what)
    return ids


@pytest.mark.parametrize('n', SIZES)
def test_assign_against_the_reference_and_the_host_twin(n):
    for name, keys in mixes(n, KNOWN).items():
        g, h, ref = three()
        assign3(g, h, ref, KNOWN, 'seed')
        ids = assign3(g, h, ref, keys, name)
        assert torch.equal(g.lookup(tt(keys)), ids), name               # every key is known now
        assert torch.equal(g.assign(tt(keys)), ids), name + ' (again)'
        same_map(g, h, ref, name + ' (again)')


def heavy_duplicates():
    rs = np.random.RandomState(11)
    distinct = (1 << 41) + rs.permutation(1 << 16)[:64].astype(np.int64) * 1000003
    return rs.permutation(np.repeat(distinct, 128))


def test_every_new_key_claimed_from_many_workgroups():
    batch = heavy_duplicates()
    assert batch.shape == (8192,) and len(np.unique(batch)) == 64
    runs = []
    for _ in range(2):
        g, h, ref = three()
        assign3(g, h, ref, KNOWN, 'seed')
        ids = assign3(g, h, ref, batch, 'heavy duplicates')
        assert g.size == len(KNOWN) + 1 + 64
        runs.append((ids, g.key_of[:g.size].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_chains_that_wrap_past_the_end_of_the_table():
    keys = keys_at_home(63, 64, 20)
    g, h, ref = three(64)
    for i, batch in enumerate(collision_batches(keys)):
        assign3(g, h, ref, batch, f'batch {i}')
    assert g.capacity == 64
    used = torch.nonzero(g.slot_key != INT64_MIN).flatten().tolist()
    assert used == list(range(19)) + [63]
    every = np.concatenate(collision_batches(keys))
    assert torch.equal(g.lookup(tt(every)).cpu(), torch.from_numpy(ref.lookup(every)))
    assert g.lookup(tt(keys_at_home(63, 64, 25)[20:])).tolist() == [-1] * 5


def test_growth_doubles_the_capacity_and_keeps_every_lookup():
    g, h, ref = IdMap(dev(), capacity=16, reserve=8), IdMap('cpu', capacity=16, reserve=8), RefMap()
    caps, every = [], np.zeros(0, dtype=np.int64)
    for b in range(5):
        keys = (1000 * (b + 1) + np.arange(7)).astype(np.int64) * 104729
        assign3(g, h, ref, keys, f'batch {b}')
        every = np.concatenate([every, keys])
        caps.append(g.capacity)
        assert torch.equal(g.lookup(tt(every)).cpu(), torch.from_numpy(ref.lookup(every)))
    assert caps == [16, 32, 64, 64, 128] and g.size == 36


def test_batch_cut_invariance():
    stream, runs = cut_stream()   # the host file's stream and cuts: 1 x 300, 300 x 1 (one launch per key), ragged
    want = RefMap()
    want_ids = torch.from_numpy(want.assign(stream))
    for name, cuts in runs.items():
        g = IdMap(dev(), capacity=16)
        ids = torch.cat([g.assign(tt(stream[a:b])) for a, b in zip(cuts[:-1], cuts[1:])])
        assert torch.equal(ids.cpu(), want_ids), name
        assert g.size == want.size and torch.equal(g.key_of[:g.size].cpu(), torch.from_numpy(want.key_of())), name


def test_batch_cut_invariance_across_tiles():
    rs = np.random.RandomState(3)
    stream = rs.randint(0, 1500, size=6000).astype(np.int64) * 2654435761 - 77
    stream[[5, 150, 4000]] = INT64_MIN
    want = RefMap()
    want_ids = torch.from_numpy(want.assign(stream))
    for name, cuts in {'one batch': [0, 6000], 'ragged': [0, 40, 100, 104, 105, 180, 2300, 2301, 4400, 6000],
                       'by 300': list(range(0, 6001, 300))}.items():
        g = IdMap(dev(), capacity=16)
        ids = torch.cat([g.assign(tt(stream[a:b])) for a, b in zip(cuts[:-1], cuts[1:])])
        assert torch.equal(ids.cpu(), want_ids), name
        assert g.size == want.size and torch.equal(g.key_of[:g.size].cpu(), torch.from_numpy(want.key_of())), name


def test_lookup_changes_nothing():
    g, h, ref = three()
    assign3(g, h, ref, KNOWN, 'seed')
    before = [t.clone() for t in g.tables]
    keys = np.concatenate([KNOWN, [INT64_MIN, 123, -123], np.arange(5000) + (1 << 50), KNOWN[::-1]]).astype(np.int64)
    ids = g.lookup(tt(keys))
    assert ids.dtype == torch.int32 and torch.equal(ids.cpu(), torch.from_numpy(ref.lookup(keys)))
    assert torch.equal(ids.cpu(), h.lookup(tt(keys, 'cpu')))
    assert g.size == ref.size and all(torch.equal(a, b) for a, b in zip(g.tables, before))
    assert g.lookup(tt([])).shape == (0,)


def test_from_keys_and_state_round_trip():
    keys = (np.arange(1, 3000).astype(np.int64) * 0x9E3779B1) ^ 0x5555
    g = IdMap.from_keys(tt(keys, 'cpu'), dev())
    assert g.size == 3000 and torch.equal(g.lookup(tt(keys)).cpu(), torch.arange(1, 3000, dtype=torch.int32))
    assert torch.equal(g.keys_of(torch.arange(3000, device=dev()))[1:].cpu(), tt(keys, 'cpu'))
    assert table_pairs(g) == set(zip(keys.tolist(), range(1, 3000)))
    g.assign(tt([7, keys[3], 8, 7, INT64_MIN, 9]))
    back = IdMap.from_state_dict(g.state_dict(), dev())
    assert back.size == g.size and torch.equal(back.key_of[:back.size], g.key_of[:g.size]) and table_pairs(back) == table_pairs(g)
    more = (np.arange(5000) % 1700 + (1 << 45)).astype(np.int64)
    assert torch.equal(back.assign(tt(more)), g.assign(tt(more)))
    assert back.size == g.size and torch.equal(back.key_of[:back.size], g.key_of[:g.size])


def test_states_that_are_no_mapping_are_refused_with_the_row():
    sd = IdMap.from_keys(tt(np.arange(10, 3000), 'cpu'), dev()).state_dict()

    def bad(*changes):
        out = dict(sd, key_of=sd['key_of'].clone())
        for row, value in changes:
            out['key_of'][row] = value
        return out

    for case, pattern in [(bad((2500, int(sd['key_of'][2]))), r'DUP.*row 2500\b'), (bad((3, INT64_MIN)), r'EMPTY_KEY.*row 3\b'),
                          (bad((2900, int(sd['key_of'][2])), (700, int(sd['key_of'][2500]))), r'DUP.*row 2500\b'),
                          (bad((2500, int(sd['key_of'][2])), (2400, INT64_MIN)), r'EMPTY_KEY.*row 2400\b')]:
        with pytest.raises(ValueError, match=pattern):
            IdMap.from_state_dict(case, dev())
    with pytest.raises(ValueError, match=r'DUP.*row 3\b'):
        IdMap.from_keys(tt([4, 5, 4, 5], 'cpu'), dev())


def test_the_wrapper_refuses_keys_of_another_device_or_type():
    g = IdMap(dev())
    for keys in (tt([1, 2], 'cpu'), tt([1, 2]).int(), tt([1, 2, 3, 4])[::2], tt([1, 2]).reshape(1, 2)):
        for fn in (g.assign, g.lookup):
            with pytest.raises(ValueError, match='contiguous 1-d int64'):
                fn(keys)
    assert g.size == 1
