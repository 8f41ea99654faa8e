"""The reference of the id map tests with removal: a dict, a heap of free ids and a set - the loop DESIGN 7.19 defines the
rule by - and the capacity rule restated (a purge when the used slots and the batch would pass half the table).  Nothing
of the library is used here but, in the thin callers at the end, the host twins over numpy arrays."""
import ctypes as C
import heapq

import numpy as np

from _idmap_ref import INT64_MIN, np_struct

INT32_MAX = (1 << 31) - 1


class RefFreeMap:
    """for x in keys: if x not in d: d[x] = heappop(free) if free else size (and size += 1)"""

    def __init__(self, capacity=16):
        self.d = {}            # key -> id (the padding key is not in it)
        self.free = []         # heap of the released ids
        self.size = 1          # the high-water mark, the padding id included
        self.capacity, self.slots_used = capacity, 1

    @property
    def n_free(self):
        return len(self.free)

    def _room(self, n):
        """the capacity rule: a rebuild when slots_used + n passes half the table, into the smallest power of two >= the
        present capacity that keeps live + n at most half full"""
        if 2 * (self.slots_used + n) > self.capacity:
            live = self.size - len(self.free)
            while 2 * (live + n) > self.capacity:
                self.capacity *= 2
            self.slots_used = live

    def assign(self, keys, return_new=False):
        self._room(len(keys))
        out, new = [], []
        for x in keys:
            x = int(x)
            if x == INT64_MIN:
                out.append(0)
                continue
            if x not in self.d:
                if self.free:
                    self.d[x] = heapq.heappop(self.free)
                else:
                    self.d[x] = self.size
                    self.size += 1
                self.slots_used += 1
                new.append(self.d[x])
            out.append(self.d[x])
        out = np.array(out, dtype=np.int32).reshape(-1)
        return (out, np.array(new, dtype=np.int32).reshape(-1)) if return_new else out

    def remove(self, keys):
        """-> ids (what every copy had before the call), the distinct released ids ascending"""
        ids = [0 if int(x) == INT64_MIN else self.d.get(int(x), -1) for x in keys]
        gone = sorted({i for i in ids if i > 0})
        for x in keys:
            self.d.pop(int(x), None)
        for i in gone:
            heapq.heappush(self.free, i)
        return np.array(ids, dtype=np.int32).reshape(-1), np.array(gone, dtype=np.int32).reshape(-1)

    def lookup(self, keys):
        return np.array([0 if int(x) == INT64_MIN else self.d.get(int(x), -1) for x in keys], dtype=np.int32).reshape(-1)

    def key_of(self):
        out = np.full(self.size, INT64_MIN, dtype=np.int64)
        for k, v in self.d.items():
            out[v] = k
        return out

    def pairs(self):
        return set(self.d.items())


def live_pairs(slot_key, slot_id):
    """the table as a set of (key, id) over the slots that hold an id: a slot of a removed key keeps its key with id -1 and
    is not part of the mapping; where a key sits may depend on the race for a slot, what it maps to may not"""
    slot_key, slot_id = np.asarray(slot_key), np.asarray(slot_id)
    assert (slot_id[slot_key == INT64_MIN] == -1).all()
    assert ((slot_id >= 1) | (slot_id == -1)).all(), 'a slot was left pending'
    used = slot_id >= 1
    out = set(zip(slot_key[used].tolist(), slot_id[used].tolist()))
    assert len(out) == int(used.sum()), 'a key sits in two slots'
    keys = slot_key[slot_key != INT64_MIN]
    assert len(set(keys.tolist())) == len(keys), 'a key sits in two slots'
    return out


def bits_to_ids(free_bits, size):
    """the set bits of a bitmap held as int64 words -> ids, ascending"""
    words = np.asarray(free_bits).view(np.uint64)
    bits = np.unpackbits(words.view(np.uint8), bitorder='little')
    ids = np.nonzero(bits)[0]
    assert (ids < size).all() and (ids >= 1).all(), 'a bit outside [1, size)'
    return ids


def fresh_keys(count, start):
    """`count` distinct keys no other call of this function with another `start` gives (start: a multiple of 2^32)"""
    return (np.arange(count, dtype=np.int64) * 2654435761 + 12345) % (1 << 31) * 3 + np.int64(start)


# ---- the host twins over numpy arrays ----------------------------------------------------------------------------------
def np_bits(key_rows):
    return np.zeros((key_rows + 63) // 64, dtype=np.int64)


def host_remove(t, size, bits, keys, capacity=None, words=None):
    """-> rc, ids, released, (n released, error bits)"""
    from www2023tiger_amd._lib import lib, ptr
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    ids, rel, out2 = np.full(len(keys), -7, dtype=np.int32), np.full(len(keys), -7, dtype=np.int32), np.full(2, -7, dtype=np.int64)
    m = np_struct(t, capacity)
    rc = lib.tg_idmap_remove_host(C.byref(m), size, ptr(bits), len(bits) if words is None else words, ptr(keys), len(keys),
                                  ptr(ids), ptr(rel), ptr(out2))
    return rc, ids, rel, (int(out2[0]), int(out2[1]))


def host_assign_recycle(t, size, occupied, bits, n_free, keys, capacity=None, words=None):
    """-> rc, ids, free_list, (size + n_new, error bits)"""
    from www2023tiger_amd._lib import lib, ptr
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    ids, out2 = np.full(len(keys), -7, dtype=np.int32), np.full(2, -7, dtype=np.int64)
    fl = np.full(max(min(n_free, len(keys)), 1), -7, dtype=np.int32)
    m = np_struct(t, capacity)
    rc = lib.tg_idmap_assign_recycle_host(C.byref(m), size, occupied, ptr(bits), len(bits) if words is None else words, n_free,
                                          ptr(keys), len(keys), ptr(ids), ptr(fl), ptr(out2))
    return rc, ids, fl, (int(out2[0]), int(out2[1]))
