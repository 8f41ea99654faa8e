"""Mirror of tiger/model/memory.py: `Memory` and `MessageStoreNoGradLastOnly`.

The dict-of-lists stores (MessageStore, MessageStoreNoGrad) are unreachable in the
reference (init_utils.py:166 hard-codes msg_last_only=True) and are not built.
State lives in torch buffers with the reference's names so checkpoints interchange;
the Python set `nodes_with_messages` becomes a device bitmap (`has_msg_bits`).
"""
import copy
from typing import Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor, nn

from .. import hip_ops
from .utils import select_latest_nids


def grow_capacity(n0: int, n: int, reserve: Optional[int]) -> int:
    """rows of a new backing store for a table that grows from n0 to n rows: `reserve` (>= n) or half as many again"""
    if reserve is not None:
        reserve = int(reserve)
        if reserve < n:
            raise ValueError(f'grow: reserve = {reserve} rows is below the {n} rows asked for')
        return reserve
    return max(n, n0 + max(16, n0 // 2))


def grow_table(mod: nn.Module, name: str, rows: int, cap_rows: int) -> bool:
    """Buffer `name` of `mod` becomes the leading `rows`-row view of a ZEROED backing store of at least cap_rows rows
    (kept in mod._stores) -> whether its data pointer moved.  While the store has room nothing is copied and no pointer
    moves: the rows at and beyond the old view are zero because the store was born zeroed and every kernel bounds the
    ids it writes by the n_nodes of the struct it is handed.  A buffer that was moved or replaced since
    (.to(), load_memory_state) no longer heads its store and gets a new one."""
    cur = getattr(mod, name)
    stores = mod.__dict__.setdefault('_stores', {})
    store = stores.get(name)
    if (store is None or store.device != cur.device or store.data_ptr() != cur.data_ptr() or store.shape[0] < cur.shape[0]
            or store.shape[0] < rows):
        store = torch.zeros((max(cap_rows, rows),) + tuple(cur.shape[1:]), dtype=cur.dtype, device=cur.device)
        store[:cur.shape[0]] = cur
        stores[name] = store
    setattr(mod, name, store[:rows])
    return getattr(mod, name).data_ptr() != cur.data_ptr()


def compact_tables(tables, old_of: Tensor, reserve: Optional[int] = None):
    """The first half of a compaction of per-node tables (TIGE.compact_nodes): tables = (module, buffer name)
    pairs, at most 8, every buffer with a row per OLD node id; old_of int32 [n_new], ascending - the old id of every new
    one.  Each buffer gets a NEW zeroed backing store with the head-room of `grow_capacity` (reserve=: its rows) whose
    leading n_new rows are store[j] = buffer[old_of[j]], all of them moved by ONE launch (hip_ops.node_rows_compact).
    Nothing of the modules has changed yet -> what `adopt_tables` swaps in.  Peak memory is old table + new table."""
    n_new = old_of.numel()
    cap = grow_capacity(n_new, n_new, reserve)
    built, pairs = [], []
    for mod, name in tables:
        cur = getattr(mod, name)
        store = torch.zeros((cap,) + tuple(cur.shape[1:]), dtype=cur.dtype, device=cur.device)
        built.append((mod, name, store, n_new))
        pairs.append((cur, store[:n_new]))
    hip_ops.node_rows_compact(pairs, old_of)
    return built


def adopt_tables(built):
    """The second half: every buffer becomes the leading view of its new store (plain attribute stores: nothing can raise)"""
    for mod, name, store, rows in built:
        mod.__dict__.setdefault('_stores', {})[name] = store
        setattr(mod, name, store[:rows])


def _old_of(what: str, mod, old_of) -> Tensor:
    if not (torch.is_tensor(old_of) and old_of.dtype == torch.int32 and old_of.dim() == 1 and old_of.is_contiguous()
            and old_of.device == mod.device and 1 <= old_of.numel() <= mod.n):
        raise ValueError(f'{what}: old_of must be a contiguous 1-d int32 tensor of 1 to {mod.n} old ids on {mod.device}')
    return old_of


class Memory(nn.Module):
    def __init__(self, n, dim):
        super().__init__()
        self.n = n
        self.dim = dim
        self.register_buffer('vals', torch.zeros(n, dim), persistent=True)
        self.register_buffer('update_ts', torch.zeros(n), persistent=True)
        self.register_buffer('active_mask', torch.zeros(n).bool(), persistent=True)
        self._version_ = 0  # bumped by every mutating method (the model's eager-update table watches it)

    def clone(self):
        """memory.py:21-25 - like the reference, active_mask is not carried over."""
        other = Memory(self.n, self.dim).to(self.device)
        other.vals.copy_(self.vals)
        other.update_ts.copy_(self.update_ts)
        return other

    @property
    def device(self):
        return self.vals.device

    def clear(self, nids: Optional[Tensor] = None):
        """Zero state, as in a freshly built Memory: every row (memory.py:31-34), or - nids: int64 ids, duplicates are
        fine - the rows of those ids alone (TIGE.erase; memory.py has no counterpart)."""
        self._version_ += 1
        if nids is None:
            self.vals.zero_()
            self.update_ts.zero_()
            self.active_mask.zero_()
            return
        if len(nids) == 0:
            return
        nids = nids.to(self.device).long().reshape(-1)
        if int(nids.min()) < 0 or int(nids.max()) >= self.n:
            raise ValueError(f'Memory.clear: a node id outside [0, {self.n})')
        self.vals.index_fill_(0, nids, 0)
        self.update_ts.index_fill_(0, nids, 0)
        self.active_mask.index_fill_(0, nids, False)

    def grow(self, n: int, reserve: Optional[int] = None) -> bool:
        """Rows for node ids [self.n, n): zero state, as in a freshly built Memory(n, dim) (online admission of new ids,
        TIGE.grow_nodes; memory.py has no counterpart: the reference sizes its tables once) -> whether a data pointer
        moved.  vals, update_ts and active_mask stay buffers of exactly n rows under their names (state_dict and
        checkpoints interchange with a module born with n rows); each is the leading view of a backing store that grows
        by half (reserve=: rows of a new store), so most calls copy nothing.  ValueError: n < self.n (rows are never
        released), reserve < n."""
        n = int(n)
        if n < self.n:
            raise ValueError(f'Memory.grow: {n} rows is fewer than the {self.n} the table has (rows are never released)')
        cap = grow_capacity(self.n, n, reserve)
        moved = [grow_table(self, name, n, cap) for name in ('vals', 'update_ts', 'active_mask')]
        self.n = n
        self._version_ += 1
        return any(moved)

    COMPACT_TABLES = ('vals', 'update_ts', 'active_mask')

    def compact(self, old_of: Tensor, reserve: Optional[int] = None):
        """Keep the rows of the ids old_of (int32, ascending: NodeCompaction.old_of), renumbered densely (TIGE.compact_nodes;
        memory.py has no counterpart: the reference sizes its tables once).  vals, update_ts and active_mask become the
        leading views of NEW zeroed backing stores with the head-room of `grow_capacity` (reserve=: their rows) and stay
        buffers of exactly old_of.numel() rows under their names: `grow` keeps working and a checkpoint interchanges with
        a module born with that many rows.  One launch moves the three tables.  ValueError: old_of is no int32 list of 1
        to n ids on the module's device, reserve below its length."""
        built = compact_tables([(self, name) for name in self.COMPACT_TABLES], _old_of('Memory.compact', self, old_of), reserve)
        self._adopt_compacted(built)

    def _adopt_compacted(self, built):
        adopt_tables(built)
        self.n = built[0][3]
        self._version_ += 1

    def get(self, ids: Tensor) -> Tuple[Tensor, Tensor]:
        return hip_ops.gather_rows(self.vals, ids, self.update_ts)

    def set(self, ids: Tensor, vals: Tensor, ts: Tensor, skip_check=False):
        if len(ids) == 0:
            return
        self._version_ += 1
        err = None
        if not skip_check:
            if len(ids) != len(torch.unique(ids)):
                raise ValueError('Duplicate node ids are not allowed.')
            err = hip_ops.new_err(self.device)
        hip_ops.memory_scatter(self.vals, self.update_ts, self.active_mask, ids, vals.detach(), ts,
                               check_past=not skip_check, err=err)
        if err is not None:
            hip_ops.raise_if_err(err)


class MessageStoreNoGradLastOnly(nn.Module):
    """Last-message mailbox: one raw message row [own | other | edge | time] per node."""

    def __init__(self, n, dim):
        super().__init__()
        self.n = n
        self.dim = dim
        self.register_buffer('node_msg_vals', torch.zeros((n, dim)).float(), persistent=False)
        self.register_buffer('node_msg_ts', torch.zeros(n).float(), persistent=False)
        self.register_buffer('has_msg_bits', torch.zeros(hip_ops.bitmap_words(n), dtype=torch.int64), persistent=False)
        self._version_ = 0  # bumped by every mutating method

    @property
    def node_messages(self):
        return (self.node_msg_vals, self.node_msg_ts)

    @property
    def device(self):
        return self.node_msg_vals.device

    def clone(self):
        return copy.deepcopy(self)

    def grow(self, n: int, reserve: Optional[int] = None) -> bool:
        """Rows for node ids [self.n, n): no message, as in a freshly built store (Memory.grow: the same contract) -> whether
        a data pointer moved.  has_msg_bits gets bitmap_words(n) words; the spare bits of the old last word are zero
        already (tg_bitmap_mark and the step bound ids by n_nodes)."""
        n = int(n)
        if n < self.n:
            raise ValueError(f'MessageStoreNoGradLastOnly.grow: {n} rows is fewer than the {self.n} the mailbox has '
                             '(rows are never released)')
        cap = grow_capacity(self.n, n, reserve)
        moved = [grow_table(self, name, n, cap) for name in ('node_msg_vals', 'node_msg_ts')]
        if moved[0]:  # the rows got a new store: the bitmap gets one of the same capacity (its old one may still have room)
            self.__dict__.get('_stores', {}).pop('has_msg_bits', None)
        moved.append(grow_table(self, 'has_msg_bits', hip_ops.bitmap_words(n), hip_ops.bitmap_words(cap)))
        self.n = n
        self._version_ += 1
        return any(moved)

    COMPACT_TABLES = ('node_msg_vals', 'node_msg_ts')

    def compact(self, old_of: Tensor, reserve: Optional[int] = None):
        """Keep the mailbox rows of the ids old_of, renumbered densely (Memory.compact: the same contract).  has_msg_bits
        becomes the bitmap over the new ids - new bit j = old bit old_of[j], spare bits zero (tg_bitmap_compact) - at the
        head of a store of the same capacity as the rows."""
        old_of = _old_of('MessageStoreNoGradLastOnly.compact', self, old_of)
        built = compact_tables([(self, name) for name in self.COMPACT_TABLES], old_of, reserve)
        self._adopt_compacted(built, self._compacted_bits(old_of, built[0][2].shape[0]))

    def _compacted_bits(self, old_of: Tensor, cap_rows: int) -> Tensor:
        store = torch.zeros(hip_ops.bitmap_words(cap_rows), dtype=torch.int64, device=self.device)
        hip_ops.bitmap_compact(self.has_msg_bits, old_of, self.n, old_of.numel(), out=store)
        return store

    def _adopt_compacted(self, built, bits_store: Tensor):
        adopt_tables(built + [(self, 'has_msg_bits', bits_store, hip_ops.bitmap_words(built[0][3]))])
        self.n = built[0][3]
        self._version_ += 1

    # -- set view of the bitmap (host sync; diagnostic / compatibility only) --------
    def _has_msg_numpy(self) -> np.ndarray:
        words = self.has_msg_bits.cpu().numpy().view(np.uint64)
        bits = np.unpackbits(words.view(np.uint8), bitorder='little')[:self.n]
        return np.nonzero(bits)[0]

    @property
    def nodes_with_messages(self) -> set:
        return set(self._has_msg_numpy().tolist())

    def get_outdated_node_ids(self, node_ids: Union[Tensor, np.ndarray, None]) -> Tensor:
        """memory.py:108-126: ids (a subset of node_ids) that hold an unconsumed message,
        as a CPU LongTensor (sorted here; the reference returns Python-set order)."""
        has = self._has_msg_numpy()
        if node_ids is not None:
            ids = node_ids if isinstance(node_ids, np.ndarray) else node_ids.cpu().numpy()
            has = np.intersect1d(has, ids)
        return torch.from_numpy(has.astype(np.int64))

    def clear(self, nids: Optional[Tensor] = None):
        """memory.py:128-138 (the reference's zero-fill of rows is a no-op on an indexed copy;
        only membership changes)."""
        self._version_ += 1
        if nids is None:
            self.has_msg_bits.zero_()
            return
        if len(nids) == 0:
            return
        nids = nids.to(self.device).long()
        mask = torch.zeros_like(self.has_msg_bits)
        hip_ops.bitmap_mark(nids, mask, self.n)
        self.has_msg_bits &= ~mask

    def store_events(self, src_ids, dst_ids, src_prev_ts, dst_prev_ts, src_vals, dst_vals, eids, ts, emb_getter,
                     time_encoder):
        """memory.py:77-106, composed from the standalone ops.  TIGE.store_events uses the
        fused tg_store_events kernel instead; this form exists for API compatibility."""
        self._version_ += 1
        pos = torch.cat([src_ids, dst_ids])
        if bool((self._bits_of(pos)).any()):
            raise ValueError('Node has unused messages.')
        sv = src_vals + emb_getter.get_node_embeddings(src_ids)
        dv = dst_vals + emb_getter.get_node_embeddings(dst_ids)
        ev = emb_getter.get_edge_embeddings(eids)
        full = torch.cat([torch.cat([sv, dv, ev, time_encoder(ts - src_prev_ts)], 1),
                          torch.cat([dv, sv, ev, time_encoder(ts - dst_prev_ts)], 1)], 0)
        ts2 = ts.repeat(2)
        ids, index = select_latest_nids(pos, ts2, self.n)
        hip_ops.memory_scatter(self.node_msg_vals, self.node_msg_ts, None, ids, full, ts2, src_index=index)
        hip_ops.bitmap_mark(ids, self.has_msg_bits, self.n)

    def has_msg_mask(self) -> Tensor:
        """bool[n] on the device: node holds an unconsumed message (the bitmap, one flag per node)"""
        return self._bits_of(torch.arange(self.n, device=self.device)).bool()

    def _bits_of(self, ids: Tensor) -> Tensor:
        return (self.has_msg_bits[ids >> 6] >> (ids & 63)) & 1
