"""Event keys without a GPU: the host twins tg_events_screen_host / tg_events_repack_host and EventKeys on the CPU against
the Python dict the screen is defined by (tests/_events_ref.py) - rows, kept positions and key_of bit for bit -, the state
round trip and every load refusal.  Integer work: no tolerance anywhere."""
import io

import numpy as np
import pytest
import torch

from _events_ref import (ERR_KEY, INT64_MIN, bits_of, commit_ref, key_mixes, repack_ref, rows_of_bits, same_home_keys,
                         screen_ref)
from www2023tiger_amd import hip_ops
from www2023tiger_amd._lib import TG_EINVAL, TigerHipError, lib, ptr
from www2023tiger_amd.data.events import EventKeys

ONE_MAX = 256
SIZES = [0, 1, 2, 63, 64, 65, ONE_MAX - 1, ONE_MAX, ONE_MAX + 1, 2047, 2048, 2049, 4097]
KNOWN = (np.arange(1, 301, dtype=np.int64) * 1_000_003) ^ 0x5DEECE66D   # the keys of rows 1 .. 300


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))


def seeded(device='cpu'):
    ev = EventKeys(device, 1 + KNOWN.size, tt(KNOWN))
    return ev, {int(k): i + 1 for i, k in enumerate(KNOWN)}


def table_bits(ev):
    return [t.cpu().clone() for t in (ev.slot_key, ev.slot_id, ev.key_of, ev.keyless)]


def check_screen(ev, d, keys, what):
    before = table_bits(ev)
    want_eids, want_keep, bad = screen_ref(d, ev.size, keys)
    run = hip_ops.events_screen_host if ev.device.type == 'cpu' else hip_ops.events_screen
    eids, keep, err = run(ev.tables, ev.size, tt(keys).to(ev.device))
    assert err == (ERR_KEY if bad else 0), what
    np.testing.assert_array_equal(eids.cpu().numpy(), want_eids, err_msg=what)
    np.testing.assert_array_equal(keep.cpu().numpy(), want_keep, err_msg=what)
    for a, b in zip(before, table_bits(ev)):
        assert torch.equal(a, b), what   # read-only on the map
    return eids, keep


def chained(n, ev):
    """n keys, each twice at most, that share ONE home slot of the scratch table of a batch of n"""
    scap = 16
    while scap < 2 * n:
        scap *= 2
    uniq = same_home_keys(lib, min(n, 40), scap - 1, home=scap - 3)   # (the chain wraps past the end of the table)
    return uniq[np.arange(n) % max(uniq.size, 1)] if n else uniq[:0]


@pytest.mark.parametrize('n', SIZES)
def test_screen_host_equals_the_dict(n):
    ev, d = seeded()
    rng = np.random.default_rng(n)
    mixes = key_mixes(n, KNOWN, rng)
    mixes['chained'] = chained(n, ev)
    for name, keys in mixes.items():
        check_screen(ev, d, keys, f'{name}, n = {n}')


def test_int64_min_in_the_batch_is_reported_and_writes_only_minus_one():
    ev, d = seeded()
    keys = np.array([5, INT64_MIN, 5, KNOWN[3], INT64_MIN, 6], dtype=np.int64)
    eids, keep = check_screen(ev, d, keys, 'INT64_MIN')
    assert eids.tolist() == [301, -1, 301, 4, -1, 302] and keep.tolist() == [0, 5]
    with pytest.raises(ValueError, match='KEY'):
        ev.screen(tt(keys))
    assert ev.size == 301


def test_the_entry_refuses_before_it_runs():
    ev, _ = seeded()
    m, _ = hip_ops._idmap_struct('t', ev.tables)
    import ctypes as C
    keys, eids, keep, out2 = tt([1, 2]), torch.empty(2, dtype=torch.int32), torch.empty(2, dtype=torch.int64), torch.empty(2, dtype=torch.int64)
    call = lambda rows, n, k=keys, e=eids, kp=keep, o=out2: lib.tg_events_screen_host(C.byref(m), rows, ptr(k), n, ptr(e), ptr(kp), ptr(o))
    assert call(ev.size, 2) == 0
    assert call(0, 2) == TG_EINVAL and call(ev.size, -1) == TG_EINVAL and call(0x7fffffff, 1) == TG_EINVAL
    assert call(ev.key_of.numel() + 1, 0) == TG_EINVAL
    assert call(ev.size, 2, None) == TG_EINVAL and call(ev.size, 2, keys, None) == TG_EINVAL
    assert call(ev.size, 2, keys, eids, None) == TG_EINVAL and call(ev.size, 2, keys, eids, keep, None) == TG_EINVAL
    assert lib.tg_events_screen_workspace_bytes(-1) == 0
    a16 = lambda x: (x + 15) // 16 * 16
    for n, tiles, scap in ((0, 0, 0), (256, 1, 0), (257, 1, 1024), (4097, 3, 16384)):
        want = 2 * a16(4 * n) + a16(256 * tiles) + 2 * a16(4 * tiles) + a16(4 * (tiles + 1)) + 12 * scap
        assert lib.tg_events_screen_workspace_bytes(n) == want, n
    with pytest.raises(ValueError, match='live on'):
        hip_ops.events_screen(ev.tables, ev.size, keys)   # CPU tables: the host twin is asked for by name
    kn, ko = torch.empty(4, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    rm = torch.zeros(4, dtype=torch.int32)
    assert lib.tg_events_repack_host(ptr(kn), ptr(ko), ptr(rm), 4, ptr(kn), ptr(ko), 5) == TG_EINVAL
    assert lib.tg_events_repack_host(ptr(kn), ptr(ko), ptr(rm), 0, ptr(kn), ptr(ko), 1) == TG_EINVAL
    assert lib.tg_events_repack_host(None, ptr(ko), ptr(rm), 4, ptr(kn), ptr(ko), 1) == TG_EINVAL


def remaps(rows_before):
    """name -> remap int32 [rows_before] (monotone, row 0 kept)"""
    r = np.arange(rows_before)
    keep = {'nothing released': np.ones(rows_before, bool), 'all but row 0': r == 0, 'alternating': r % 2 == 0,
            'a block at a word edge': ~((r >= 60) & (r < 130)), 'a long run': ~((r >= 3) & (r < rows_before - 2))}
    out = {}
    for name, k in keep.items():
        k = k.copy()
        k[0] = True
        out[name] = np.where(k, np.cumsum(k) - 1, -1).astype(np.int32)
    return out


def check_repack(rows_before, device='cpu'):
    rng = np.random.default_rng(rows_before)
    key_of = rng.integers(1, 1 << 62, rows_before, dtype=np.int64)
    keyless = np.flatnonzero(rng.random(rows_before) < 0.4)
    keyless = keyless[keyless > 0]
    key_of[keyless] = INT64_MIN
    key_of[0] = INT64_MIN
    run = hip_ops.events_repack_host if device == 'cpu' else hip_ops.events_repack
    for name, remap in remaps(rows_before).items():
        rows_new = int(remap.max()) + 1
        want_keys, want_keyless = repack_ref(key_of, keyless, remap, rows_new)
        new_keys = torch.full((rows_new + 7,), 77, dtype=torch.int64, device=device)
        new_bits = torch.full(((rows_new + 63) // 64 + 1,), 0x55, dtype=torch.int64, device=device)
        run(tt(key_of).to(device), tt(bits_of(keyless, rows_before)).to(device), torch.from_numpy(remap).to(device), rows_before,
            new_keys, new_bits, rows_new)
        what = f'{name}, rows_before = {rows_before}'
        np.testing.assert_array_equal(new_keys[:rows_new].cpu().numpy(), want_keys, err_msg=what)
        assert bool((new_keys[rows_new:] == 77).all()) and int(new_bits[-1]) == 0x55, what   # nothing beyond is written
        np.testing.assert_array_equal(rows_of_bits(new_bits[:-1].cpu().numpy(), 64 * (new_bits.numel() - 1)), want_keyless,
                                      err_msg=what)


@pytest.mark.parametrize('rows_before', [1, 64, 65, 2049])
def test_repack_host_equals_the_scatter(rows_before):
    check_repack(rows_before)


def test_eventkeys_on_the_cpu_screen_commit_released_and_round_trip():
    ev, d = seeded()
    rng = np.random.default_rng(7)
    rows = ev.size
    for step in range(6):   # growth on the way: 301 -> ~ 2 700 rows
        n = (5, 300, 64, 1000, 257, 900)[step]
        fresh = rng.integers(1, 1 << 40, n, dtype=np.int64)
        keys = np.where(rng.random(n) < 0.3, KNOWN[rng.integers(0, KNOWN.size, n)], fresh)
        keys[n // 2:] = np.where(rng.random(n - n // 2) < 0.3, keys[:n - n // 2], keys[n // 2:])   # in-batch copies
        want_eids, want_keep, _ = screen_ref(d, rows, keys)
        eids, keep = ev.screen(tt(keys))
        np.testing.assert_array_equal(eids.numpy(), want_eids)
        np.testing.assert_array_equal(keep.numpy(), want_keep)
        assert ev.size == rows   # the screen changed nothing ...
        ev.reserve(keep.numel())
        ev.commit(tt(keys)[keep])
        rows = commit_ref(d, rows, keys[want_keep])
        assert ev.size == rows
        again, nothing = ev.screen(tt(keys))   # ... and the same batch again keeps nothing and names the committed rows
        assert nothing.numel() == 0
        np.testing.assert_array_equal(again.numpy(), want_eids)
        np.testing.assert_array_equal(ev.lookup(tt(keys)).numpy(), want_eids)
    np.testing.assert_array_equal(ev.keys_of(torch.arange(rows)).numpy()[1:], np.array(sorted(d, key=d.get), dtype=np.int64))
    with pytest.raises(RuntimeError, match='not what screen kept'):
        EventKeys('cpu', 3, tt([8, 9])).commit(tt([9, 10]))

    # a release: every third row leaves
    from www2023tiger_amd.model.feature_getter import EdgeRowsRelease
    live = np.arange(rows) % 3 != 1
    live[0] = True
    remap = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
    res = EdgeRowsRelease(torch.from_numpy(remap), None, rows, int(live.sum()), None)
    all_keys = np.array(sorted(d, key=d.get), dtype=np.int64)
    ev.released(res)
    assert ev.size == int(live.sum()) and ev.n_keyless == 0
    got = ev.lookup(tt(all_keys)).numpy()
    np.testing.assert_array_equal(got, remap[1:])   # a released key is unknown, a kept key maps to remap[old]
    with pytest.raises(ValueError, match='release covers'):
        ev.released(res)   # (a release of another table: nothing changes)
    assert ev.size == int(live.sum())

    # the state round trip, through a file, weights_only
    f = io.BytesIO()
    torch.save(ev.state_dict(), f)
    f.seek(0)
    back = EventKeys.from_state_dict(torch.load(f, weights_only=True), 'cpu')
    assert back.size == ev.size and back.n_keyless == 0
    assert torch.equal(back.key_of[:back.size], ev.key_of[:ev.size])
    np.testing.assert_array_equal(back.lookup(tt(all_keys)).numpy(), got)
    probe = tt(np.concatenate([all_keys[:50], np.arange(1, 60, dtype=np.int64) << 41]))
    for a, b in zip(back.screen(probe), ev.screen(probe)):
        assert torch.equal(a, b)


def test_keyless_rows_are_never_matched_and_follow_a_release():
    ev = EventKeys('cpu', 130)   # a model built on 129 events nobody named
    assert ev.size == 130 and ev.n_keyless == 129
    assert ev.keyless_rows().tolist() == list(range(1, 130))
    keys = tt(np.arange(10, 80, dtype=np.int64))
    eids, keep = ev.screen(keys)
    assert keep.tolist() == list(range(70)) and eids.tolist() == list(range(130, 200))
    ev.commit(keys)
    assert ev.size == 200 and ev.lookup(keys).tolist() == list(range(130, 200))
    from www2023tiger_amd.model.feature_getter import EdgeRowsRelease
    live = np.ones(200, bool)
    live[5:70] = False    # keyless rows leave across a word edge
    live[131:140] = False
    remap = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
    ev.released(EdgeRowsRelease(torch.from_numpy(remap), None, 200, int(live.sum()), None))
    assert ev.size == int(live.sum()) and ev.n_keyless == 129 - 65
    assert ev.keyless_rows().tolist() == list(range(1, 129 - 65 + 1))
    np.testing.assert_array_equal(ev.lookup(keys).numpy(), remap[130:200])
    back = EventKeys.from_state_dict(ev.state_dict(), 'cpu')
    assert back.n_keyless == ev.n_keyless and back.keyless_rows().tolist() == ev.keyless_rows().tolist()
    np.testing.assert_array_equal(back.lookup(keys).numpy(), remap[130:200])
    assert bool((back.keys_of(torch.arange(1, 65)) == INT64_MIN).all())


def test_what_the_constructor_and_a_load_refuse():
    with pytest.raises(ValueError, match='rows'):
        EventKeys('cpu', 0)
    with pytest.raises(ValueError, match='one key for each'):
        EventKeys('cpu', 4, tt([1, 2]))
    with pytest.raises(ValueError, match='DUP.*row 3'):
        EventKeys('cpu', 5, tt([7, 8, 7, 9]))
    with pytest.raises(ValueError, match='EMPTY_KEY.*row 2'):
        EventKeys('cpu', 4, tt([7, INT64_MIN, 9]))
    good = EventKeys('cpu', 6, tt([11, 12, 13, 14, 15])).state_dict()
    assert good['format'] == 'tiger-event-keys' and good['keyless'].numel() == 0
    load = lambda **kw: EventKeys.from_state_dict({**good, **kw}, 'cpu')
    assert load().size == 6
    with pytest.raises(ValueError, match='not saved event keys'):
        load(format='tiger-idmap')
    with pytest.raises(ValueError, match='not saved event keys'):
        EventKeys.from_state_dict([1], 'cpu')
    with pytest.raises(ValueError, match='version 2'):
        load(version=2)
    with pytest.raises(ValueError, match='key_of must be'):
        load(key_of=good['key_of'].int())
    with pytest.raises(ValueError, match=r'key_of\[0\]'):
        load(key_of=tt([1, 2, 3]))
    with pytest.raises(ValueError, match='keyless must be a 1-d'):
        load(keyless=None)
    with pytest.raises(ValueError, match=r'ascend.*entry 2'):
        load(keyless=tt([1, 3, 3]))
    with pytest.raises(ValueError, match='outside'):
        load(keyless=tt([6]))
    with pytest.raises(ValueError, match='outside'):
        load(keyless=tt([0, 1]))
    with pytest.raises(ValueError, match='DUP.*row 4'):   # a duplicate key, the smallest row that repeats one
        load(key_of=tt([INT64_MIN, 11, 12, 13, 12, 11]))
    with pytest.raises(ValueError, match='EMPTY_KEY.*row 2'):   # a stray INT64_MIN
        load(key_of=tt([INT64_MIN, 11, INT64_MIN, 13, 14, 15]))
    with pytest.raises(ValueError, match='FREE.*row 3'):   # bitmap and row disagree: a keyless row that holds a key
        load(keyless=tt([3]))
    with pytest.raises(ValueError, match='EMPTY_KEY.*row 2'):   # ... and the smallest of several offenders is named
        load(key_of=tt([INT64_MIN, 11, INT64_MIN, 13, 14, 15]), keyless=tt([4]))
    ok = load(key_of=tt([INT64_MIN, 11, INT64_MIN, 13, 14, 15]), keyless=tt([2]))
    assert ok.n_keyless == 1 and ok.lookup(tt([11, 13, 15])).tolist() == [1, 3, 5]
