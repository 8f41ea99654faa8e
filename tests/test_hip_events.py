"""Event keys on the GPU: tg_events_screen / tg_events_repack against the Python dict (tests/_events_ref.py) AND against
their host twins, bit for bit - at the wavefront, one-workgroup-bound and tile edges, past one chunk of the base scan
(n > 256 * 2048), for every key mix of the host test, with probe chains in the scratch table; the persistent tables are
bit-identical before and after a screen."""
import numpy as np
import pytest
import torch

from _events_ref import ERR_KEY, INT64_MIN, commit_ref, key_mixes, screen_ref
from test_events_host import KNOWN, SIZES, chained, check_repack, check_screen, seeded, tt
from www2023tiger_amd import hip_ops
from www2023tiger_amd.data.events import EventKeys

pytestmark = pytest.mark.gpu
BIG = 256 * 2048 + 1 + 5   # 257 tiles: the base scan crosses a chunk of 256


def dev():
    return torch.device('cuda', 0)


def host_twin(ev, keys):
    tables = tuple(t.cpu() for t in ev.tables)
    return hip_ops.events_screen_host(tables, ev.size, tt(keys))


def check_both(ev, d, keys, what):
    eids, keep = check_screen(ev, d, keys, what)   # the dict; the tables before and after
    h_eids, h_keep, _ = host_twin(ev, keys)
    assert torch.equal(eids.cpu(), h_eids) and torch.equal(keep.cpu(), h_keep), what
    return eids, keep


@pytest.mark.parametrize('n', SIZES)
def test_screen_equals_the_dict_and_the_host_twin(n):
    ev, d = seeded(dev())
    rng = np.random.default_rng(n)
    mixes = key_mixes(n, KNOWN, rng)
    mixes['chained'] = chained(n, ev)
    for name, keys in mixes.items():
        check_both(ev, d, keys, f'{name}, n = {n}')


def test_screen_past_one_chunk_of_the_base_scan():
    ev, d = seeded(dev())
    mixes = key_mixes(BIG, KNOWN, np.random.default_rng(1))
    for name in ('new', 'twice', 'interleaved'):
        eids, keep = check_both(ev, d, mixes[name], f'{name}, n = {BIG}')
    assert int(keep[-1]) > 256 * 2048   # (interleaved: a first occurrence in the last tile gets its base from chunk 2)


def test_int64_min_is_reported_and_writes_only_minus_one():
    ev, d = seeded(dev())
    for n in (6, 300):
        keys = np.arange(n, dtype=np.int64) % 4 + 5
        keys[[1, n - 2]] = INT64_MIN
        keys[3] = KNOWN[3]
        eids, keep = check_both(ev, d, keys, f'INT64_MIN, n = {n}')
        assert eids[1] == -1 and eids[n - 2] == -1 and int(eids[3]) == 4
        with pytest.raises(ValueError, match='KEY'):
            ev.screen(tt(keys).to(dev()))
    assert ev.size == 301


def test_screen_commit_screen_keeps_nothing_and_growth_keeps_the_mapping():
    ev, d = seeded(dev())
    rng = np.random.default_rng(3)
    rows = ev.size
    for n in (40, 256, 257, 3000):
        fresh = rng.integers(1, 1 << 40, n, dtype=np.int64)
        keys = np.where(rng.random(n) < 0.3, KNOWN[rng.integers(0, KNOWN.size, n)], fresh)
        keys[n // 2:] = np.where(rng.random(n - n // 2) < 0.3, keys[:n - n // 2], keys[n // 2:])
        k = tt(keys).to(dev())
        want_eids, want_keep, _ = screen_ref(d, rows, keys)
        eids, keep = ev.screen(k)
        np.testing.assert_array_equal(eids.cpu().numpy(), want_eids)
        np.testing.assert_array_equal(keep.cpu().numpy(), want_keep)
        ev.reserve(keep.numel())
        ev.commit(k[keep])
        rows = commit_ref(d, rows, keys[want_keep])
        assert ev.size == rows
        again, nothing = ev.screen(k)
        assert nothing.numel() == 0
        np.testing.assert_array_equal(again.cpu().numpy(), want_eids)
    all_keys = np.array(sorted(d, key=d.get), dtype=np.int64)
    np.testing.assert_array_equal(ev.lookup(tt(all_keys).to(dev())).cpu().numpy(), np.arange(1, rows))
    back = EventKeys.from_state_dict(ev.state_dict(), dev())
    assert back.size == rows and torch.equal(back.key_of[:rows], ev.key_of[:rows])


@pytest.mark.parametrize('rows_before', [1, 64, 65, 2049])
def test_repack_equals_the_scatter(rows_before):
    check_repack(rows_before, dev())


def test_after_a_release_a_released_key_is_unknown_and_a_kept_key_follows_its_row():
    from www2023tiger_amd.model.feature_getter import EdgeRowsRelease
    rows = 2049
    keys = np.arange(1, rows, dtype=np.int64) * 31 + 7
    for keyless in (False, True):
        ev = EventKeys(dev(), rows, None if keyless else tt(keys))
        if keyless:   # the rows the model was built with have no key; 500 keyed rows follow
            ev.commit(tt(keys[:500]).to(dev()))
        size = ev.size
        r = np.arange(size)
        live = (r % 5 != 2) & ~((r >= 60) & (r < 130))
        live[0] = True
        remap = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
        first = rows if keyless else 1   # the first keyed row
        held = keys[:size - first]
        host = EventKeys.from_state_dict(ev.state_dict(), 'cpu')
        for e in (ev, host):
            e.released(EdgeRowsRelease(torch.from_numpy(remap).to(e.device), None, size, int(live.sum()), None))
        assert ev.size == int(live.sum()) == host.size and ev.n_keyless == host.n_keyless
        np.testing.assert_array_equal(ev.lookup(tt(held).to(dev())).cpu().numpy(), remap[first:size])
        assert torch.equal(ev.key_of[:ev.size].cpu(), host.key_of[:host.size])
        assert ev.keyless_rows().tolist() == host.keyless_rows().tolist()
        if keyless:
            assert ev.keyless_rows().tolist() == remap[1:rows][live[1:rows]].tolist()
