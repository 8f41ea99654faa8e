"""EventKeys: external 64-bit event keys -> rows of the model's edge-feature table, on the device (tiger_hip.h:
tg_events_*).

The reference names an event by its row in the data set and has no counterpart of this.  A served model meets
transaction ids: a message bus delivers a batch twice, a client retries after a time-out, a chargeback names the
transaction it cancels.  The tracker follows the edge table through its whole life - rows appended by `observe_events`,
rows released and renumbered by `forget` / `erase` / `release_edge_rows` - so the caller keeps no dictionary of what it
has sent and translates no row numbers (TIGE.track_events / observe_events / retract_events)."""
from typing import Optional

import torch
from torch import Tensor

from .. import hip_ops
from .idmap import INT64_MIN, MAX_SIZE, _capacity_for

FORMAT, VERSION = 'tiger-event-keys', 1


def _bit_rows(words: Tensor, size: int) -> Tensor:
    """the set bits below `size` of a bitmap of 64-bit words -> int64, ascending, on the CPU"""
    words = words[:(size + 63) // 64].cpu()
    bits = (words.unsqueeze(1) >> torch.arange(64)) & 1
    return torch.nonzero(bits.reshape(-1)[:size]).reshape(-1)


class EventKeys:
    """The map and its size.  THE INVARIANT: `size` == the rows of the model's edge table, always; row 0 is the padding
    row, its key INT64_MIN.  slot_key / slot_id / key_of are a tg_idmap whose dense ids are edge rows (key_of: row -> key);
    `keyless`: the device bitmap of rows that have no key (bit r set <=> key_of[r] == INT64_MIN, 1 <= r < size) - rows the
    model was built with when no keys were given for them: never matched, never retractable by key.
    EventKeys(device, rows, keys=None): keys int64 [rows - 1] name the rows 1 .. rows - 1; None: they are keyless.
    ValueError: a key that stands twice, or INT64_MIN, naming the row.
    device 'cpu' runs the library's host twins over the same layout (tests, tools); there is no other fallback.
    THE LIMITS: a key lives as long as its edge row - after a release of that row a redelivered copy is an unknown event
    again; the map is saved whole (8 B per row, `state_dict`) beside the model's online state: journal deltas do not
    carry it."""

    def __init__(self, device, rows: int, keys: Optional[Tensor] = None):
        rows = int(rows)
        if rows < 1 or rows > MAX_SIZE:
            raise ValueError(f'EventKeys: rows = {rows} must lie in [1, 2^31 - 1] (the padding row included)')
        key_of = torch.full((rows,), INT64_MIN, dtype=torch.int64)
        keyless = None
        if keys is None:
            keyless = torch.arange(1, rows, dtype=torch.int64)
        else:
            keys = torch.as_tensor(keys)
            if keys.dtype != torch.int64 or keys.dim() != 1 or keys.numel() != rows - 1:
                raise ValueError(f'EventKeys: keys must be a 1-d int64 tensor with one key for each of the rows 1 .. {rows - 1}')
            key_of[1:] = keys.cpu()
        self._install('EventKeys', key_of, keyless, device)

    def _install(self, what: str, key_of: Tensor, keyless: Optional[Tensor], device):
        """become the map of key_of [size] (CPU) with the keyless rows `keyless` (CPU int64, ascending, or None)"""
        size = key_of.numel()
        n_keyless = 0 if keyless is None else keyless.numel()
        key_rows = max(size, 16)
        slot_key, slot_id, dev_key_of = hip_ops.idmap_tables(_capacity_for(size), key_rows, torch.device(device))
        dev = slot_key.device
        dev_key_of[:size] = key_of.to(dev)
        bits = hip_ops.idmap_free_bits(key_rows, dev)
        if n_keyless:
            flags = torch.zeros(bits.numel() * 64, dtype=torch.int64)
            flags[keyless] = 1
            bits.copy_((flags.view(-1, 64) << torch.arange(64)).sum(1))   # (bit 63: the sum wraps to the sign bit, as meant)
            err = hip_ops.idmap_rebuild_free((slot_key, slot_id, dev_key_of), size, size - n_keyless, bits)
        else:
            err = hip_ops.idmap_rebuild((slot_key, slot_id, dev_key_of), size)
        if err:
            raise ValueError(f'{what}: ' + hip_ops.IDMAP_ERR_TEXT(err))
        self.device = dev
        self.slot_key, self.slot_id, self.key_of, self.keyless = slot_key, slot_id, dev_key_of, bits
        self.size, self.n_keyless = size, n_keyless

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
            raise ValueError(f'EventKeys.{what}: keys must be a contiguous 1-d int64 tensor on {self.device}')
        return keys

    def _rebuilt(self, capacity: int, key_rows: int, key_of: Tensor, keyless: Tensor, size: int, n_keyless: int):
        """fresh tables of `capacity` slots over key_of[:size] (already of key_rows rows) - nothing is read back: the keys
        of a map are distinct"""
        slot_key, slot_id, _ = hip_ops.idmap_tables(capacity, 1, self.device)
        if n_keyless:
            hip_ops.idmap_rebuild_free((slot_key, slot_id, key_of), size, size - n_keyless, keyless, read_back=False)
        else:
            hip_ops.idmap_rebuild((slot_key, slot_id, key_of), size, read_back=False)
        return slot_key, slot_id

    def reserve(self, n: int):
        """room for n more rows (IdMap._grow): the table is rebuilt at twice the capacity (or more) when size + n would pass
        half of it, key_of and the bitmap grow by half when size + n would pass their end.  The MAPPING does not change.
        `observe_events` calls it before the batch is observed, so that `commit` cannot fail for want of room."""
        from ..model.memory import grow_capacity
        need = self.size + int(n)
        if need > MAX_SIZE:
            raise ValueError(f'EventKeys: {self.size} rows and {n} events would pass 2^31 - 1 rows')
        rows = self.key_of.numel()
        rebuild = 2 * need > self.capacity
        if not rebuild and need <= rows:
            return
        key_of, keyless = self.key_of, self.keyless
        if need > rows:
            new_rows = min(grow_capacity(rows, need, None), MAX_SIZE)
            key_of = torch.full((new_rows,), INT64_MIN, dtype=torch.int64, device=self.device)
            key_of[:self.size] = self.key_of[:self.size]
            keyless = hip_ops.idmap_free_bits(new_rows, self.device)
            keyless[:self.keyless.numel()] = self.keyless
        if rebuild:
            slot_key, slot_id = self._rebuilt(_capacity_for(need, self.capacity), key_of.numel(), key_of, keyless, self.size,
                                              self.n_keyless)
            self.slot_key, self.slot_id = slot_key, slot_id
        self.key_of, self.keyless = key_of, keyless

    def screen(self, keys: Tensor):
        """What of a batch is new -> (eids int32 [n], keep int64 [m]); THE MAP IS NOT CHANGED.  Equivalent to
            d = the map; kept = []
            for i, k in enumerate(keys):
                if k not in d: d[k] = size + len(kept); kept.append(i)
                eids[i] = d[k]
        with d thrown away: keep = the positions of the first occurrences of the keys the map does not hold, ascending -
        the events to observe, which will get the rows size, size + 1, ...; eids[i] = the row of keys[i]: the stored row
        of a key seen before, the row of its first copy for a duplicate inside the batch.  ONE read-back (m and the error
        word).  ValueError: keys that are no contiguous 1-d int64 tensor on the map's device, INT64_MIN among them, a
        size that would pass 2^31 - 1.  RuntimeError: a table this library did not make."""
        keys = self._keys('screen', keys)
        if self.size + keys.numel() > MAX_SIZE:
            raise ValueError(f'EventKeys.screen: {self.size} rows and {keys.numel()} events would pass 2^31 - 1 rows')
        run = hip_ops.events_screen_host if self.device.type == 'cpu' else hip_ops.events_screen
        eids, keep, err = run(self.tables, self.size, keys)
        if err & hip_ops.EVENTS_ERR_KEY:
            raise ValueError('EventKeys.screen: ' + hip_ops.EVENTS_ERR_TEXT(err))
        if err:
            raise RuntimeError('EventKeys.screen: ' + hip_ops.EVENTS_ERR_TEXT(err))
        return eids, keep

    def commit(self, kept_keys: Tensor):
        """The keys of the events a screened batch kept (keys[keep]: distinct, unknown to the map), AFTER their rows were
        appended to the edge table: they get the rows size, size + 1, ... in order (tg_idmap_assign) and size grows by
        their number.  RuntimeError - and a map that no longer mirrors the table - if a key was known or stood twice:
        commit what `screen` kept, once."""
        kept_keys = self._keys('commit', kept_keys)
        m = kept_keys.numel()
        if m == 0:
            return
        self.reserve(m)
        _, size, err = hip_ops.idmap_assign(self.tables, self.size, kept_keys)
        if err:
            raise RuntimeError('EventKeys.commit: ' + hip_ops.IDMAP_ERR_TEXT(err))
        grown, self.size = size - self.size, size
        if grown != m:
            raise RuntimeError(f'EventKeys.commit: {m - grown} of the {m} keys were known to the map or stood twice - they '
                               'are not what screen kept')

    def lookup(self, keys: Tensor) -> Tensor:
        """-> rows int32 [n]: -1 for a key the map does not hold (0 for INT64_MIN, the key of the padding row).  Never
        changes the map, reads nothing back."""
        return hip_ops.idmap_lookup(self.tables, self._keys('lookup', keys))

    def keys_of(self, eids: Tensor, check: bool = True) -> Tensor:
        """-> keys int64, of the shape of eids (a gather of key_of; INT64_MIN for the padding row and for a keyless row).
        ValueError: a row outside [0, size) (one read-back; check=False for rows the model itself returned)."""
        eids = torch.as_tensor(eids, device=self.device)
        if eids.dtype not in (torch.int32, torch.int64):
            raise ValueError('EventKeys.keys_of: eids are int32 or int64')
        if check and eids.numel() and bool(((eids < 0) | (eids >= self.size)).any()):
            raise ValueError(f'EventKeys.keys_of: a row outside [0, {self.size})')
        return self.key_of[eids.long()]

    def keyless_rows(self) -> Tensor:
        """-> the rows without a key, int64, ascending, on the CPU (read from the bitmap: state files, tools)"""
        return _bit_rows(self.keyless, self.size)

    def released(self, res):
        """Follow a release of edge rows (res: the EdgeRowsRelease of NumericalFeature.compact_edge_rows): the key of a
        kept row moves to remap[row] (tg_events_repack), the keys of released rows leave, and the table is rebuilt over
        the new rows.  Everything is built first and swapped in one step: if the call raises, the map has not changed.
        ValueError: a release of a table with another number of rows, or on another device."""
        self._adopt(self._released_build(res))

    def _released_build(self, res):
        remap = res.remap
        if res.rows_before != self.size or remap.device != self.device or remap.numel() != self.size:
            raise ValueError(f'EventKeys.released: the release covers {res.rows_before} rows on {remap.device}, the map '
                             f'{self.size} on {self.device}')
        rows = int(res.rows)
        key_rows = max(rows + max(16, rows // 4), 16)   # (head-room as the packed edge table has)
        key_of = torch.full((key_rows,), INT64_MIN, dtype=torch.int64, device=self.device)
        keyless = hip_ops.idmap_free_bits(key_rows, self.device)
        run = hip_ops.events_repack_host if self.device.type == 'cpu' else hip_ops.events_repack
        run(self.key_of, self.keyless, remap.contiguous(), self.size, key_of, keyless, rows)
        n_keyless = 0
        if self.n_keyless:   # (one read-back, and only for a map that began with keyless rows)
            n_keyless = int(_bit_rows(keyless, rows).numel())
        slot_key, slot_id = self._rebuilt(_capacity_for(rows), key_rows, key_of, keyless, rows, n_keyless)
        return slot_key, slot_id, key_of, keyless, rows, n_keyless

    def _adopt(self, built):
        self.slot_key, self.slot_id, self.key_of, self.keyless, self.size, self.n_keyless = built

    def state_dict(self) -> dict:
        """The MAPPING: key_of[:size] on the CPU, the keyless rows (int64, ascending) and a format tag (loads with
        torch.load(weights_only=True)).  The table is rebuilt on load.  Saved beside `TIGE.online_state()`, whole."""
        return {'format': FORMAT, 'version': VERSION, 'key_of': self.key_of[:self.size].cpu().clone(),
                'keyless': self.keyless_rows()}

    @classmethod
    def from_state_dict(cls, state: dict, device) -> 'EventKeys':
        """ValueError: no saved event keys, another version, a key_of that is no 1-d int64 tensor headed by INT64_MIN, a
        `keyless` that is no 1-d int64 tensor, not strictly ascending (naming the entry) or outside [1, size); and - found
        by tg_idmap_rebuild / _rebuild_free, naming the smallest row - a key that stands twice (DUP), INT64_MIN in a row
        that is not keyless (EMPTY_KEY), a keyless row that holds a key (FREE)."""
        what = 'EventKeys.from_state_dict'
        if not isinstance(state, dict) or state.get('format') != FORMAT:
            raise ValueError(f'{what}: not saved event keys')
        if state.get('version') != VERSION:
            raise ValueError(f'{what}: version {state.get("version")} (this library reads version {VERSION})')
        key_of = state.get('key_of')
        if not torch.is_tensor(key_of) or key_of.dtype != torch.int64 or key_of.dim() != 1 or key_of.numel() < 1:
            raise ValueError(f'{what}: key_of must be a 1-d int64 tensor with the padding row')
        if key_of.numel() > MAX_SIZE:
            raise ValueError(f'{what}: {key_of.numel()} rows would pass 2^31 - 1')
        if int(key_of[0]) != INT64_MIN:
            raise ValueError(f'{what}: key_of[0] must be INT64_MIN, the key of the padding row')
        keyless = state.get('keyless')
        if not torch.is_tensor(keyless) or keyless.dtype != torch.int64 or keyless.dim() != 1:
            raise ValueError(f'{what}: keyless must be a 1-d int64 tensor (the rows without a key)')
        keyless = keyless.cpu()
        if keyless.numel():
            unsorted = torch.nonzero(keyless[1:] <= keyless[:-1]).reshape(-1)
            if unsorted.numel():
                raise ValueError(f'{what}: keyless must ascend without duplicates (entry {int(unsorted[0]) + 1})')
            if int(keyless[0]) < 1 or int(keyless[-1]) >= key_of.numel():
                raise ValueError(f'{what}: a keyless row outside [1, {key_of.numel()})')
        self = cls.__new__(cls)
        self._install(what, key_of.cpu(), keyless if keyless.numel() else None, device)
        return self
