"""IdMap: external 64-bit keys -> the model's dense node ids, on the device (tiger_hip.h: tg_idmap).

The reference numbers its nodes offline (its preprocessing script writes dense ids into the data set) and has no
counterpart of this.  A served model meets account numbers and hashes; the map turns them into row numbers without a host
dictionary, deterministically: a key the map does not hold gets the next id in the order of first appearance - what
`for x in keys: d.setdefault(x, len(d))` gives - so a stream gets the same ids however it is cut into batches."""
from typing import Optional

import torch
from torch import Tensor

from .. import hip_ops

INT64_MIN = hip_ops.IDMAP_EMPTY
MAX_SIZE = 0x7FFFFFFF          # dense ids are int32
FORMAT, VERSION = 'tiger-idmap', 1


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
    device 'cpu' runs the library's host twins over the same layout (tests, tools); there is no other fallback.
    Not built: removing a key (after TIGE.erase the key stays mapped to its emptied row), recycling ids, keys for eids."""

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
        self.size = 1

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
        """room for `need` ids: the capacity doubles until 2 * need fits and the table is rebuilt from key_of (the host
        knows the size and that its keys are distinct: nothing is read back); key_of grows by half, like Memory.grow - on
        its own, by a copy, while the capacity still fits"""
        from ..model.memory import grow_capacity
        cap = _capacity_for(need, self.capacity)
        rows = self.key_of.numel()
        if cap == self.capacity and need <= rows:
            return
        new_rows = min(grow_capacity(rows, need, None), MAX_SIZE) if need > rows else rows
        if cap == self.capacity:   # only key_of is too short: the table stays as it is
            key_of = torch.full((new_rows,), INT64_MIN, dtype=torch.int64, device=self.device)
            key_of[:self.size] = self.key_of[:self.size]
            self.key_of = key_of
            return
        slot_key, slot_id, key_of = hip_ops.idmap_tables(cap, new_rows, self.device)
        key_of[:self.size] = self.key_of[:self.size]
        hip_ops.idmap_rebuild((slot_key, slot_id, key_of), self.size, read_back=False)
        self.slot_key, self.slot_id, self.key_of = slot_key, slot_id, key_of

    def assign(self, keys: Tensor) -> Tensor:
        """lookup-or-insert -> ids int32 [n] on the device.  A key the map does not hold gets size + the rank of its first
        occurrence among the first occurrences of all such keys; size is updated from the call's ONE read-back.  The
        tables grow first when the batch could pass half the capacity or the end of key_of.  ValueError before any
        launch: keys that are no contiguous 1-d int64 tensor on the map's device, a size that would pass 2^31 - 1."""
        keys = self._keys('assign', keys)
        need = self.size + keys.numel()
        if need > MAX_SIZE:
            raise ValueError(f'IdMap.assign: {self.size} ids and {keys.numel()} keys would pass 2^31 - 1 dense ids')
        self._grow(need)
        ids, size, err = hip_ops.idmap_assign(self.tables, self.size, keys)
        if err:
            raise RuntimeError('IdMap.assign: ' + hip_ops.IDMAP_ERR_TEXT(err))
        self.size = size
        return ids

    def lookup(self, keys: Tensor) -> Tensor:
        """-> ids int32 [n]: -1 for a key the map does not hold, 0 for INT64_MIN.  Never changes the map, reads nothing
        back."""
        return hip_ops.idmap_lookup(self.tables, self._keys('lookup', keys))

    def keys_of(self, ids: Tensor, check: bool = True) -> Tensor:
        """-> keys int64, of the shape of ids (a gather of key_of; id 0 gives INT64_MIN).  ValueError: an id outside
        [0, size) (one read-back; check=False for ids the model itself returned)."""
        ids = torch.as_tensor(ids, device=self.device)
        if ids.dtype not in (torch.int32, torch.int64):
            raise ValueError('IdMap.keys_of: ids are int32 or int64')
        if check and ids.numel() and bool(((ids < 0) | (ids >= self.size)).any()):
            raise ValueError(f'IdMap.keys_of: an id outside [0, {self.size})')
        return self.key_of[ids.long()]

    @classmethod
    def _from_rows(cls, what: str, key_of: Tensor, device, capacity: Optional[int]) -> 'IdMap':
        size = key_of.numel()
        if size > MAX_SIZE:
            raise ValueError(f'{what}: {size} rows would pass 2^31 - 1 dense ids')
        self = cls(device, _capacity_for(size, capacity or 16), reserve=max(size, 16))
        self.key_of[:size] = key_of.to(self.device)
        err = hip_ops.idmap_rebuild(self.tables, size)
        if err:
            raise ValueError(f'{what}: ' + hip_ops.IDMAP_ERR_TEXT(err))
        self.size = size
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
        rebuilt on load, so the restored map assigns exactly as this one would."""
        return {'format': FORMAT, 'version': VERSION, 'key_of': self.key_of[:self.size].cpu().clone()}

    @classmethod
    def from_state_dict(cls, state: dict, device, capacity: Optional[int] = None) -> 'IdMap':
        """ValueError: no saved id map, another version, a key_of that is no 1-d int64 tensor headed by INT64_MIN, and - found
        by tg_idmap_rebuild - a key that stands twice or INT64_MIN in a row >= 1, naming the row."""
        if not isinstance(state, dict) or state.get('format') != FORMAT:
            raise ValueError('IdMap.from_state_dict: not a saved id map')
        if state.get('version') != VERSION:
            raise ValueError(f'IdMap.from_state_dict: version {state.get("version")} (this library reads version {VERSION})')
        key_of = state.get('key_of')
        if not torch.is_tensor(key_of) or key_of.dtype != torch.int64 or key_of.dim() != 1 or key_of.numel() < 1:
            raise ValueError('IdMap.from_state_dict: key_of must be a 1-d int64 tensor with the padding row')
        if int(key_of[0]) != INT64_MIN:
            raise ValueError('IdMap.from_state_dict: key_of[0] must be INT64_MIN, the key of the padding id')
        return cls._from_rows('IdMap.from_state_dict', key_of, device, capacity)
