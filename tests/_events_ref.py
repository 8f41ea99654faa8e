"""Plain-Python references for the event-key tests (test_events_host.py, test_hip_events.py, test_hip_events_model.py):
dicts and loops, integer only - every comparison against them is bit-exact."""
import ctypes

import numpy as np

INT64_MIN = -(1 << 63)
ERR_KEY = 32   # tiger_hip.h: TG_EVENTS_ERR_KEY


def screen_ref(d: dict, rows: int, keys):
    """tg_events_screen over the mapping d (key -> row): -> (eids int32 [n], keep int64 [m], INT64_MIN seen).  d is not
    modified."""
    d = dict(d)
    kept, eids, bad = [], [], False
    for i, k in enumerate(int(x) for x in keys):
        if k == INT64_MIN:
            eids.append(-1)
            bad = True
            continue
        if k not in d:
            d[k] = rows + len(kept)
            kept.append(i)
        eids.append(d[k])
    return np.asarray(eids, dtype=np.int32), np.asarray(kept, dtype=np.int64), bad


def commit_ref(d: dict, rows: int, kept_keys) -> int:
    """the kept keys get rows, rows + 1, ... -> the new row count"""
    for j, k in enumerate(int(x) for x in kept_keys):
        assert k not in d
        d[k] = rows + j
    return rows + len(kept_keys)


def repack_ref(key_of_old, keyless_old_rows, remap, rows_new: int):
    """tg_events_repack as a numpy scatter -> (key_of_new [rows_new], keyless rows of the new table, ascending)"""
    key_of_old, remap = np.asarray(key_of_old), np.asarray(remap)
    key_of_new = np.full(rows_new, INT64_MIN, dtype=np.int64)
    live = remap >= 0
    key_of_new[remap[live]] = key_of_old[:remap.size][live]
    flag = np.zeros(remap.size, dtype=bool)
    flag[np.asarray(keyless_old_rows, dtype=np.int64)] = True
    return key_of_new, np.sort(remap[live & flag]).astype(np.int64)


def bits_of(rows_set, n_rows: int) -> np.ndarray:
    """the rows of rows_set as a bitmap of 64-bit words (int64 storage) over n_rows rows"""
    words = np.zeros((n_rows + 63) // 64, dtype=np.uint64)
    for r in rows_set:
        words[int(r) >> 6] |= np.uint64(1) << np.uint64(int(r) & 63)
    return words.view(np.int64)


def rows_of_bits(words, n_rows: int) -> np.ndarray:
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder='little')[:n_rows]
    return np.flatnonzero(bits).astype(np.int64)


def same_home_keys(lib, count: int, mask: int, home: int = 5, start: int = 1):
    """`count` distinct positive keys whose home slot tg_idmap_hash(key) & mask is `home`: one probe chain"""
    lib.tg_idmap_hash.restype = ctypes.c_uint64
    lib.tg_idmap_hash.argtypes = [ctypes.c_int64]
    out, k = [], start
    while len(out) < count:
        if lib.tg_idmap_hash(k) & mask == home:
            out.append(k)
        k += 1
    return np.asarray(out, dtype=np.int64)


def key_mixes(n: int, known: np.ndarray, rng, tile: int = 2048):
    """name -> keys int64 [n]: all new, all known, known and new interleaved, all one key, every key twice with the copies a
    tile apart (the chained one is made by the caller: it needs the library)"""
    fresh = np.arange(n, dtype=np.int64) * 7 + 1_000_000_007
    mixes = {'new': fresh.copy()}
    if known.size:
        mixes['known'] = known[rng.integers(0, known.size, n)] if n else fresh[:0]
        inter = fresh.copy()
        inter[::2] = known[rng.integers(0, known.size, inter[::2].size)]
        mixes['interleaved'] = inter
    mixes['one'] = np.full(n, 424242, dtype=np.int64)
    half = fresh[:(n + 1) // 2]
    gap = tile if n >= 2 * tile else (n + 1) // 2   # the copies a tile apart where the batch is long enough
    i = np.arange(n, dtype=np.int64)
    blk, off = np.divmod(i, 2 * max(gap, 1))
    mixes['twice'] = fresh[(blk * gap + off % max(gap, 1)) % max(half.size, 1)] if n else fresh[:0]
    return mixes
