"""IdMap: external 64-bit keys -> the model's dense node ids, on the device (tiger_hip.h: tg_idmap).

The reference numbers its nodes offline (its preprocessing script writes dense ids into the data set) and has no
counterpart of this.  A served model meets account numbers and hashes; the map turns them into row numbers without a host
dictionary, deterministically: a key the map does not hold gets the next id in the order of first appearance - what
`for x in keys: d.setdefault(x, len(d))` gives - so a stream gets the same ids however it is cut into batches.
Keys can be removed; their ids are recycled, the smallest first, so a service whose accounts come and go
stays as large as its peak of live accounts."""
from typing import Optional

import torch
from torch import Tensor

from .. import hip_ops

INT64_MIN = hip_ops.IDMAP_EMPTY
MAX_SIZE = 0x7FFFFFFF          # dense ids are int32
FORMAT, VERSION = 'tiger-idmap', 1
FORMAT_FREE, VERSION_FREE = 'tiger-idmap-free', 1   # a map with free ids: key_of with holes and the sorted free ids


def _capacity_for(size: int, at_least: int = 16) -> int:
    """the smallest power of two >= at_least that keeps `size` ids at most half full"""
    cap = max(16, int(at_least))
    while cap & (cap - 1):
        cap += cap & -cap
    while 2 * size > cap:
        cap *= 2
    return cap


class IdMap:
    """The map and its size.  slot_key / slot_id are the open-addressing table, key_of [key_rows] the reverse table (dense id
    -> key, key_of[0] = INT64_MIN: the key of the padding id 0, never inserted; looking it up or assigning it gives 0).
    size = ids in use, the padding id included: a fresh map has size 1, and size is the num_node of the model behind it.
    `remove` releases ids: size never shrinks - it is the high-water mark - and the released ids are handed out again, the
    smallest first, before size grows.  free_bits: the device bitmap of the free ids (bit i set <=> key_of[i] == INT64_MIN,
    1 <= i < size), n_free their number, slots_used a host upper bound on the table slots in use, the slots of removed keys
    and one for the padding id included: a removed slot keeps its key so that probe chains stay intact, and the table is
    rebuilt from key_of - purged of those slots, possibly at the SAME capacity - when slots_used + n would pass half of it.
    device 'cpu' runs the library's host twins over the same layout (tests, tools); there is no other fallback.
    `compact` takes the free ids out and shrinks the tables to the live keys.  Keys for EVENTS (eids) are data/events.py:
    EventKeys, over the same table layout and kernels."""

    def __init__(self, device, capacity: int = 1024, reserve: Optional[int] = None):
        self.device = torch.device(device)
        capacity = int(capacity)
        if capacity < 16 or capacity & (capacity - 1):
            raise ValueError(f'IdMap: capacity = {capacity} must be a power of two >= 16')
        key_rows = capacity // 2 if reserve is None else int(reserve)
        if key_rows < 1 or key_rows > MAX_SIZE:
            raise ValueError(f'IdMap: reserve = {key_rows} rows of key_of must lie in [1, 2^31 - 1]')
        self.slot_key, self.slot_id, self.key_of = hip_ops.idmap_tables(capacity, key_rows, self.device)
        self.device = self.slot_key.device  # ('cuda' -> 'cuda:0': what the keys' device is compared with)
        self.free_bits = hip_ops.idmap_free_bits(key_rows, self.device)
        self.size = 1
        self.n_free = 0
        self.slots_used = 1

    @property
    def capacity(self) -> int:
        return self.slot_key.numel()

    @property
    def tables(self):
        return self.slot_key, self.slot_id, self.key_of

    def __len__(self):
        return self.size

    def _keys(self, what: str, keys) -> Tensor:
        if not (torch.is_tensor(keys) and keys.dtype == torch.int64 and keys.dim() == 1 and keys.is_contiguous()
                and keys.device == self.device):
            raise ValueError(f'IdMap.{what}: keys must be a contiguous 1-d int64 tensor on {self.device}')
        return keys

    def _grow(self, need: int):
        """room for `need` = size + n ids, n the keys of a batch.  The table: when slots_used + n would pass half the capacity it is rebuilt from
        key_of into fresh tables of _capacity_for(live + n) slots - the capacity doubles until that fits, or stays, when
        purging the slots of removed keys is enough - and slots_used becomes the live count (the host knows the size and
        that its keys are distinct: nothing is read back).  key_of (and the bitmap with it) grows by half, like
        Memory.grow, when size + the new keys that find no free id could pass its end - on its own, by a copy, while the
        table still fits.  A map that never removed has live = slots_used = size and grows exactly as it always did."""
        from ..model.memory import grow_capacity
        n = need - self.size
        live = self.size - self.n_free
        need = self.size + max(0, n - self.n_free)
        rebuild = 2 * (self.slots_used + n) > self.capacity
        rows = self.key_of.numel()
        if not rebuild and need <= rows:
            return
        new_rows = min(grow_capacity(rows, need, None), MAX_SIZE) if need > rows else rows
        if new_rows != rows:
            free_bits = hip_ops.idmap_free_bits(new_rows, self.device)
            free_bits[:self.free_bits.numel()] = self.free_bits
            self.free_bits = free_bits
        if not rebuild:            # only key_of is too short: the table stays as it is
            key_of = torch.full((new_rows,), INT64_MIN, dtype=torch.int64, device=self.device)
            key_of[:self.size] = self.key_of[:self.size]
            self.key_of = key_of
            return
        slot_key, slot_id, key_of = hip_ops.idmap_tables(_capacity_for(live + n, self.capacity), new_rows, self.device)
        key_of[:self.size] = self.key_of[:self.size]
        if self.n_free:
            hip_ops.idmap_rebuild_free((slot_key, slot_id, key_of), self.size, live, self.free_bits, read_back=False)
        else:
            hip_ops.idmap_rebuild((slot_key, slot_id, key_of), self.size, read_back=False)
        self.slot_key, self.slot_id, self.key_of = slot_key, slot_id, key_of
        self.slots_used = live

    def assign(self, keys: Tensor, return_new: bool = False):
        """lookup-or-insert -> ids int32 [n] on the device.  With nothing free, a key the map does not hold gets size + the
        rank of its first occurrence among the first occurrences of all such keys.  With free ids (after `remove`) the new
        key of rank r gets the r-th SMALLEST free id while r < n_free and size + (r - n_free) after that - what
            for x in keys:
                if x not in d: d[x] = heappop(free) if free else size (and size += 1)
        gives; no id is freed inside a call, so a stream still gets the same ids however it is cut into batches between two
        removes.  size, n_free and slots_used are updated from the call's ONE read-back.  The tables grow first when the
        batch could pass half the capacity or the end of key_of.
        return_new=True -> (ids, new_ids): new_ids int32 = the ids given out by this call in the order of first
        appearance (the recycled ones, ascending, then the new tail range); nothing more is read back.
        ValueError before any launch: keys that are no contiguous 1-d int64 tensor on the map's device, a size that would
        pass 2^31 - 1."""
        keys = self._keys('assign', keys)
        n = keys.numel()
        if self.size + max(0, n - self.n_free) > MAX_SIZE:
            raise ValueError(f'IdMap.assign: {self.size} ids and {n} keys would pass 2^31 - 1 dense ids')
        self._grow(self.size + n)
        before = self.size
        if self.n_free == 0:
            ids, size, err = hip_ops.idmap_assign(self.tables, self.size, keys)
            n_new, recycled = size - before, None
        else:
            ids, free_list, n_new, err = hip_ops.idmap_assign_recycle(self.tables, self.size, self.slots_used, self.free_bits,
                                                                      self.n_free, keys)
            recycled = free_list[:min(n_new, self.n_free)]
        if err:
            raise RuntimeError('IdMap.assign: ' + hip_ops.IDMAP_ERR_TEXT(err))
        self.size = before + max(0, n_new - self.n_free)
        self.n_free -= min(self.n_free, n_new)
        self.slots_used += n_new
        if not return_new:
            return ids
        tail = torch.arange(before, self.size, dtype=torch.int32, device=self.device)
        return ids, (tail if recycled is None else torch.cat([recycled, tail]))

    def remove(self, keys: Tensor):
        """-> (ids int32 [n], removed_ids int32): ids[i] = the id keys[i] had - -1 for a key the map does not hold (or that
        an earlier call removed), 0 for INT64_MIN, which is never removed; every copy of a key in the batch reads the same
        id.  removed_ids = the distinct ids this call released, ascending.  A removed key is unknown to `lookup`; when it
        comes back it is a new key.  Its id is free: `assign` hands the smallest free id out first, `keys_of` gives
        INT64_MIN for it and `is_free` True.  size does not shrink.  ONE read-back: the number released."""
        keys = self._keys('remove', keys)
        ids, released, n_released, err = hip_ops.idmap_remove(self.tables, self.size, self.free_bits, keys)
        if err:
            raise RuntimeError('IdMap.remove: ' + hip_ops.IDMAP_ERR_TEXT(err))
        self.n_free += n_released
        return ids, released.sort().values[:n_released]   # (INT32_MAX at the positions that released nothing)

    def compact(self, plan=None):
        """Take the free ids out: the live ids are renumbered densely in their order -> the NodeCompaction
        (plan.translate gives the new id of an old one, -1 for a free one).  plan: a plan over THIS map's ids with drop_bits
        = free_bits (TIGE.compact_keys passes the one it made for the model: one plan serves both sides); None: made here
        (hip_ops.node_compact_plan over `size` ids without a graph; its host twin on the CPU).  key_of is gathered by
        plan.old_of and the table rebuilt by tg_idmap_rebuild at _capacity_for(n_new) slots, so capacity SHRINKS; afterwards
        size = slots_used = n_new, n_free = 0 and the bitmap is clear: the map saves the version-1 'tiger-idmap' dict
        again and `assign` hands out size, size + 1, ...  Nothing free: the identity plan, nothing changes.  Everything is
        built first and swapped in one step: if the call raises, the map has not changed.  ValueError: a plan over fewer
        ids than `size`, or one that keeps another number of ids than the map has live."""
        if plan is None:
            make = hip_ops.node_compact_host if self.device.type == 'cpu' else hip_ops.node_compact_plan
            plan = make(None, self.free_bits, self.size)
        self._compact_adopt(self._compact_build(plan))
        return plan

    def _compact_build(self, plan):
        """the new tables of `compact`, or None when nothing is free; the map has not changed"""
        live = self.size - self.n_free
        if plan.n_old < self.size or plan.rows_below(self.size) != live or plan.device != self.device:
            raise ValueError(f'IdMap.compact: the plan covers {plan.n_old} ids on {plan.device}, the map has {self.size} '
                             f'({live} live) on {self.device}')
        if self.n_free == 0:
            return None
        rows = max(live, 16)
        slot_key, slot_id, key_of = hip_ops.idmap_tables(_capacity_for(live), rows, self.device)
        hip_ops.node_rows_compact([(self.key_of, key_of[:live])], plan.old_of)
        hip_ops.idmap_rebuild((slot_key, slot_id, key_of), live, read_back=False)   # (live keys are distinct: nothing to read)
        return slot_key, slot_id, key_of, hip_ops.idmap_free_bits(rows, self.device), live

    def _compact_adopt(self, built):
        if built is not None:
            self.slot_key, self.slot_id, self.key_of, self.free_bits, live = built
            self.size, self.n_free, self.slots_used = live, 0, live

    def is_free(self, ids: Tensor) -> Tensor:
        """-> bool, of the shape of ids: the id was released and not handed out again (a gather of the bitmap).  ValueError:
        an id outside [0, size) (one read-back)."""
        ids = torch.as_tensor(ids, device=self.device)
        if ids.dtype not in (torch.int32, torch.int64):
            raise ValueError('IdMap.is_free: ids are int32 or int64')
        if ids.numel() and bool(((ids < 0) | (ids >= self.size)).any()):
            raise ValueError(f'IdMap.is_free: an id outside [0, {self.size})')
        ids = ids.long()
        return ((self.free_bits[ids >> 6] >> (ids & 63)) & 1).bool()

    def free_ids(self) -> Tensor:
        """-> the free ids, int64, ascending, on the CPU (read from the bitmap: state files, tools)"""
        words = self.free_bits[:(self.size + 63) // 64].cpu()
        bits = (words.unsqueeze(1) >> torch.arange(64)) & 1
        return torch.nonzero(bits.reshape(-1)).reshape(-1)

    def lookup(self, keys: Tensor) -> Tensor:
        """-> ids int32 [n]: -1 for a key the map does not hold, 0 for INT64_MIN.  Never changes the map, reads nothing
        back."""
        return hip_ops.idmap_lookup(self.tables, self._keys('lookup', keys))

    def keys_of(self, ids: Tensor, check: bool = True) -> Tensor:
        """-> keys int64, of the shape of ids (a gather of key_of; id 0 gives INT64_MIN, and so does a FREE id - one whose key
        was removed: INT64_MIN is no key, so it cannot be mistaken for one).  ValueError: an id outside [0, size) (one
        read-back; check=False for ids the model itself returned)."""
        ids = torch.as_tensor(ids, device=self.device)
        if ids.dtype not in (torch.int32, torch.int64):
            raise ValueError('IdMap.keys_of: ids are int32 or int64')
        if check and ids.numel() and bool(((ids < 0) | (ids >= self.size)).any()):
            raise ValueError(f'IdMap.keys_of: an id outside [0, {self.size})')
        return self.key_of[ids.long()]

    @classmethod
    def _from_rows(cls, what: str, key_of: Tensor, device, capacity: Optional[int], free: Optional[Tensor] = None) -> 'IdMap':
        size = key_of.numel()
        if size > MAX_SIZE:
            raise ValueError(f'{what}: {size} rows would pass 2^31 - 1 dense ids')
        n_free = 0 if free is None else free.numel()
        self = cls(device, _capacity_for(size - n_free, capacity or 16), reserve=max(size, 16))
        self.key_of[:size] = key_of.to(self.device)
        if n_free:
            bits = torch.zeros(self.free_bits.numel() * 64, dtype=torch.int64)
            bits[free] = 1
            words = (bits.view(-1, 64) << torch.arange(64)).sum(1)   # (bit 63: the sum wraps to the sign bit, as meant)
            self.free_bits.copy_(words)
            err = hip_ops.idmap_rebuild_free(self.tables, size, size - n_free, self.free_bits)
        else:
            err = hip_ops.idmap_rebuild(self.tables, size)
        if err:
            raise ValueError(f'{what}: ' + hip_ops.IDMAP_ERR_TEXT(err))
        self.size, self.n_free, self.slots_used = size, n_free, size - n_free
        return self

    @classmethod
    def from_keys(cls, keys, device, capacity: Optional[int] = None) -> 'IdMap':
        """keys[i] becomes dense id i + 1: a model trained on a dense data set goes behind keys without being renumbered.
        ValueError: a key that stands twice, or INT64_MIN, naming the row (= the dense id)."""
        keys = torch.as_tensor(keys)
        if keys.dtype != torch.int64 or keys.dim() != 1:
            raise ValueError('IdMap.from_keys: keys must be a 1-d int64 tensor')
        key_of = torch.cat([torch.tensor([INT64_MIN], dtype=torch.int64), keys.cpu()])
        return cls._from_rows('IdMap.from_keys', key_of, device, capacity)

    def state_dict(self) -> dict:
        """The MAPPING: key_of[:size] on the CPU and a format tag (loads with torch.load(weights_only=True)).  The table is
        rebuilt on load, so the restored map assigns exactly as this one would.  A map without free ids saves the
        'tiger-idmap' version-1 dict; one with free ids saves under 'tiger-idmap-free': key_of[:size] with INT64_MIN in the
        free rows, and `free`, the free ids (int64, ascending)."""
        key_of = self.key_of[:self.size].cpu().clone()
        if self.n_free == 0:
            return {'format': FORMAT, 'version': VERSION, 'key_of': key_of}
        return {'format': FORMAT_FREE, 'version': VERSION_FREE, 'key_of': key_of, 'free': self.free_ids()}

    @classmethod
    def from_state_dict(cls, state: dict, device, capacity: Optional[int] = None) -> 'IdMap':
        """ValueError: no saved id map, another version, a key_of that is no 1-d int64 tensor headed by INT64_MIN, and - found
        by tg_idmap_rebuild - a key that stands twice or INT64_MIN in a row >= 1, naming the row.  A 'tiger-idmap-free'
        state also: a `free` that is no 1-d int64 tensor, empty, not strictly ascending (naming the entry) or outside
        [1, size); a free id whose row holds a key (FREE) and INT64_MIN in a row that is not free (EMPTY_KEY), naming the
        smallest such row."""
        fmt = state.get('format') if isinstance(state, dict) else None
        if fmt not in (FORMAT, FORMAT_FREE):
            raise ValueError('IdMap.from_state_dict: not a saved id map')
        reads = VERSION if fmt == FORMAT else VERSION_FREE
        if state.get('version') != reads:
            raise ValueError(f'IdMap.from_state_dict: version {state.get("version")} (this library reads version {reads})')
        key_of = state.get('key_of')
        if not torch.is_tensor(key_of) or key_of.dtype != torch.int64 or key_of.dim() != 1 or key_of.numel() < 1:
            raise ValueError('IdMap.from_state_dict: key_of must be a 1-d int64 tensor with the padding row')
        if int(key_of[0]) != INT64_MIN:
            raise ValueError('IdMap.from_state_dict: key_of[0] must be INT64_MIN, the key of the padding id')
        free = None
        if fmt == FORMAT_FREE:
            free = state.get('free')
            if not torch.is_tensor(free) or free.dtype != torch.int64 or free.dim() != 1 or free.numel() < 1:
                raise ValueError('IdMap.from_state_dict: free must be a non-empty 1-d int64 tensor (the free ids)')
            free = free.cpu()
            unsorted = torch.nonzero(free[1:] <= free[:-1]).reshape(-1)
            if unsorted.numel():
                raise ValueError(f'IdMap.from_state_dict: free must ascend without duplicates (entry {int(unsorted[0]) + 1})')
            if int(free[0]) < 1 or int(free[-1]) >= key_of.numel():
                raise ValueError(f'IdMap.from_state_dict: a free id outside [1, {key_of.numel()})')
        return cls._from_rows('IdMap.from_state_dict', key_of, device, capacity, free)
