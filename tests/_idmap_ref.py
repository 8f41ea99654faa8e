"""The reference of the id map tests: the Python loop the assignment rule is defined by, the header's hash restated (used
only to find keys with a given home slot - the mapping itself never depends on it), the batches every test shares, and
thin callers of the host twins over numpy arrays."""
import ctypes as C

import numpy as np

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)   # 256 / 257: the one-launch form's limit
M64 = (1 << 64) - 1


class RefMap:
    """`for x in keys: d.setdefault(x, len(d))` with INT64_MIN as the key of the padding id 0"""

    def __init__(self):
        self.d = {INT64_MIN: 0}

    @property
    def size(self):
        return len(self.d)

    def assign(self, keys):
        return np.array([self.d.setdefault(int(x), len(self.d)) for x in keys], dtype=np.int32).reshape(-1)

    def lookup(self, keys):
        return np.array([self.d.get(int(x), -1) for x in keys], dtype=np.int32).reshape(-1)

    def key_of(self):
        out = np.empty(len(self.d), dtype=np.int64)
        for k, v in self.d.items():
            out[v] = k
        return out


def ref_hash(key: int) -> int:
    """tiger_hip.h: tg_idmap_hash (the splitmix64 step)"""
    z = (key + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def keys_at_home(slot: int, capacity: int, count: int, start: int = 1):
    """the first `count` integers >= start whose home slot in a table of `capacity` slots is `slot`"""
    out, x = [], start
    while len(out) < count:
        if ref_hash(x) & (capacity - 1) == slot:
            out.append(x)
        x += 1
    return np.array(out, dtype=np.int64)


def collision_batches(keys):
    """20 keys -> 4 batches of 10 positions: 5 new keys each, every one beside another one's duplicate (a, e, b, d, c, c, d,
    b, e, a).  size + n stays <= 32, so a table of 64 slots is not grown."""
    return [np.stack([g, g[::-1]], 1).reshape(-1) for g in np.split(np.asarray(keys, dtype=np.int64), 4)]


def mixes(n: int, known: np.ndarray, seed: int = 0):
    """name -> keys int64 [n]; `known`: keys the map holds already (at least one).  Fresh keys come from a range `known`
    does not touch."""
    rs = np.random.RandomState(seed + n)
    fresh = (1 << 40) + rs.permutation(4 * n + 8)[:n].astype(np.int64) * 7919
    half = np.concatenate([fresh[:n - n // 2], fresh[:n // 2]])
    edge = np.array([0, -1, INT64_MAX, INT64_MIN + 1], dtype=np.int64)
    out = {'all-new': fresh, 'all-known': known[rs.randint(0, len(known), size=n)],
           'one-new-key': np.full(n, (1 << 50) + 3, dtype=np.int64), 'half-duplicates': rs.permutation(half),
           'edge-keys': np.resize(edge, n),
           'padding-key': np.where(np.arange(n) % 3 == 1, INT64_MIN, np.resize(known[:5], n)).astype(np.int64)}
    if n:
        pad_new = fresh.copy()
        pad_new[rs.randint(0, n, size=max(1, n // 4))] = INT64_MIN
        out['padding-among-new'] = pad_new
        out['new-and-known'] = np.where(rs.rand(n) < 0.5, fresh, known[rs.randint(0, len(known), size=n)])
    return {k: np.ascontiguousarray(v, dtype=np.int64) for k, v in out.items()}


def cut_stream():
    """one stream of 300 keys (~110 distinct, many repeats, the padding key twice) and the cuts it is assigned in:
    1 x 300, 300 x 1 and ragged -> stream, {name: batch bounds}"""
    rs = np.random.RandomState(3)
    stream = rs.randint(0, 120, size=300).astype(np.int64) * 2654435761 - 77
    stream[[5, 150]] = INT64_MIN
    return stream, {'1 x 300': [0, 300], '300 x 1': list(range(301)), 'ragged': [0, 40, 100, 104, 105, 180, 300]}


KNOWN = np.array([5, 17, -3, 1 << 33, 42, 99, -(1 << 40)], dtype=np.int64)


def pairs(slot_key, slot_id):
    """the table as a set of (key, id): where a key sits may depend on the race for a slot, what it maps to may not"""
    slot_key, slot_id = np.asarray(slot_key), np.asarray(slot_id)
    used = slot_key != INT64_MIN
    assert (slot_id[~used] == -1).all()
    out = set(zip(slot_key[used].tolist(), slot_id[used].tolist()))
    assert len(out) == int(used.sum()), 'a key sits in two slots'
    return out


# ---- the host twins over numpy arrays ----------------------------------------------------------------------------------
def np_tables(capacity, key_rows):
    return (np.full(capacity, INT64_MIN, dtype=np.int64), np.full(capacity, -1, dtype=np.int32),
            np.full(key_rows, INT64_MIN, dtype=np.int64))


def np_struct(t, capacity=None):
    from www2023tiger_amd._lib import TgIdmap, ptr
    return TgIdmap(len(t[0]) if capacity is None else capacity, len(t[2]), ptr(t[0]), ptr(t[1]), ptr(t[2]))


def host_assign(t, size, keys, capacity=None):
    """-> rc, ids, (new size, error word)"""
    from www2023tiger_amd._lib import lib, ptr
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    ids, out2 = np.full(len(keys), -7, dtype=np.int32), np.full(2, -7, dtype=np.int64)
    m = np_struct(t, capacity)
    rc = lib.tg_idmap_assign_host(C.byref(m), size, ptr(keys), len(keys), ptr(ids), ptr(out2))
    return rc, ids, (int(out2[0]), int(out2[1]))


def host_lookup(t, keys):
    from www2023tiger_amd._lib import lib, ptr
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    ids = np.full(len(keys), -7, dtype=np.int32)
    m = np_struct(t)
    assert lib.tg_idmap_lookup_host(C.byref(m), ptr(keys), len(keys), ptr(ids)) == 0
    return ids
