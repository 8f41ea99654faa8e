"""Removing keys and recycling dense ids on the GPU (tg_idmap_remove / _assign_recycle / _rebuild_free): the cases of
tests/test_idmap_free_host.py through the kernels, compared with the reference loop (tests/_idmap_free_ref.py) AND with the
host twin - ids, the ids given out, the released ids, size, key_of and the bitmap with torch.equal; the table only as a
set of (key, id) pairs, since where a key sits may depend on the race for a slot.  n = 256 / 257 are the two forms of both
entries, 2048 / 2049 a tile of positions, 4097 the scan over tile counts; ids 131 071 .. 131 073 the select's tile edge.
No test fills a table or aims at the probe bound."""
import io

import numpy as np
import pytest
import torch

import _idmap_free_cases as cases
from _idmap_free_ref import fresh_keys
from _idmap_ref import keys_at_home
from www2023tiger_amd.data.idmap import IdMap

pytestmark = pytest.mark.gpu


def both():
    return (torch.device('cuda', 0), 'cpu')


@pytest.mark.parametrize('n', cases.SIZES)
def test_assign_and_remove_against_the_reference_and_the_host_twin(n):
    cases.case_sizes(both(), n)


def test_free_ids_on_both_sides_of_a_word_edge():
    cases.case_word_edge(both())


def test_free_ids_on_both_sides_of_a_select_tile_edge():
    cases.case_tile_edge(both())


def test_remove_duplicates_unknown_keys_the_padding_key_and_keys_that_come_back():
    cases.case_remove_forms(both())


def test_a_chain_that_wraps_stays_intact_when_its_middle_is_removed():
    cases.case_wrapping_chain(both(), keys_at_home)


def test_batch_cut_invariance_between_removes():
    cases.case_cut_invariance(both())


def test_every_copy_of_a_key_from_many_workgroups_twice():
    """64 keys x 128 copies over 8192 positions through remove and through assign behind free ids: one thread per distinct
    id counts it, whatever the race, and two runs on fresh maps give the same bits"""
    runs = [cases.case_heavy_duplicates(both()) for _ in range(2)]
    for (a, ids_a), (b, ids_b) in [runs]:
        assert np.array_equal(ids_a, ids_b)
        for (key_of_a, free_a), (key_of_b, free_b) in zip(a, b):
            assert torch.equal(key_of_a, key_of_b) and torch.equal(free_a, free_b)


def test_churn_keeps_size_and_capacity_bounded():
    maps, ref = cases.make(both())
    live = fresh_keys(64, 1 << 32)
    cases.assign(maps, ref, live)
    rs = np.random.RandomState(2)
    for r in range(200):
        out = rs.permutation(64)[:16]
        cases.remove(maps, ref, live[out], f'round {r}')
        live[out] = fresh_keys(16, (r + 2) << 32)
        cases.assign(maps, ref, live[out], f'round {r}')
        assert maps[0].size <= 81 and maps[0].capacity <= 512, (r, maps[0].size, maps[0].capacity)
    cases.lookups(maps, ref, live)
    assert maps[0].capacity == ref.capacity == 256


def test_state_round_trip_with_holes_on_the_device():
    dev = both()[0]
    maps, ref = cases.make((dev,))
    keys = fresh_keys(3000, 1 << 32)
    cases.assign(maps, ref, keys)
    cases.remove(maps, ref, keys[[2, 62, 63, 64, 130, 2047, 2048, 2998]])
    f = io.BytesIO()
    torch.save(maps[0].state_dict(), f)
    f.seek(0)
    sd = torch.load(f, weights_only=True)
    assert sd['format'] == 'tiger-idmap-free' and sd['free'].tolist() == [3, 63, 64, 65, 131, 2048, 2049, 2999]
    back = IdMap.from_state_dict(sd, dev)
    assert cases.live_pairs(back.slot_key.cpu().numpy(), back.slot_id.cpu().numpy()) == ref.pairs()
    batch = np.concatenate([fresh_keys(5, 5 << 32), keys[[2, 7]], fresh_keys(400, 6 << 32)])
    cases.assign(maps, ref, batch)                       # the saved map goes on ...
    assert torch.equal(back.assign(cases.tt(batch, dev)).cpu(), torch.from_numpy(ref.lookup(batch)))   # ... and the loaded one
    assert back.size == ref.size and back.n_free == 0 and torch.equal(back.key_of[:back.size], maps[0].key_of[:ref.size])
    for rows, free, pattern in (({63: 12345}, None, r'FREE.*row 63\b'), ({1500: cases.INT64_MIN}, None, r'EMPTY_KEY.*row 1500\b'),
                                ({}, sd['free'][1:], r'EMPTY_KEY.*row 3\b'), ({2500: int(sd['key_of'][7])}, None, r'DUP.*row 2500\b'),
                                ({63: 12345, 20: cases.INT64_MIN}, None, r'EMPTY_KEY.*row 20\b')):
        case = dict(sd, key_of=sd['key_of'].clone(), free=sd['free'] if free is None else free)
        for row, value in rows.items():
            case['key_of'][row] = value
        with pytest.raises(ValueError, match=pattern):
            IdMap.from_state_dict(case, dev)
