"""Mirror of tiger/model/feature_getter.py (NumericalFeature)."""
from typing import Optional

import torch
from torch import Tensor, nn

from .. import hip_ops


class EdgeRowsRelease:
    """What a release of edge-table rows did (NumericalFeature.compact_edge_rows, TIGE.release_edge_rows).
    remap: int32 [rows_before], old row -> new row, -1 for a released row; monotone, so rows at and beyond the call's
    keep_from moved as one block: new = old - shift.  eid_out: the graph's renumbered eid array (int32, bit 31 = direction).
    rows_before / rows: table rows before and after; shift = rows_before - rows."""
    __slots__ = ('remap', 'eid_out', 'rows_before', 'rows', 'shift', '_store')

    def __init__(self, remap, eid_out, rows_before: int, rows: int, store):
        self.remap, self.eid_out = remap, eid_out
        self.rows_before, self.rows = int(rows_before), int(rows)
        self.shift = self.rows_before - self.rows
        self._store = store

    def __repr__(self):
        return f'EdgeRowsRelease(rows_before={self.rows_before}, rows={self.rows}, shift={self.shift})'


class NumericalFeature(nn.Module):
    """Raw node / edge feature tables.  A missing table means zeros of width `dim`
    (feature_getter.py:81-85,95-99).  The HIP engine reads the tables in place; the
    get_* methods are the standalone lookups (tg_gather_rows)."""

    def __init__(self, nfeats: Optional[Tensor], efeats: Optional[Tensor], dim: int, *, use_tsfm: bool = False,
                 register_buffer: bool = True, device: torch.device = None):
        super().__init__()
        if use_tsfm:
            raise NotImplementedError('use_tsfm is never enabled by init_model (init_utils.py:137-139)')
        self.pin_mem = register_buffer
        self.device = device
        self.use_tsfm = use_tsfm
        self.out_dim = dim
        self.n_nodes = self.n_edges = None
        nd = ed = None
        if nfeats is not None:
            self.n_nodes, nd = nfeats.shape
        if efeats is not None:
            self.n_edges, ed = efeats.shape
        prep = lambda t: None if t is None else t.float().contiguous()
        if register_buffer:
            # buffers are non-persistent like the reference (not part of the state_dict); they move with .to(device)
            self.register_buffer('nfeats', prep(nfeats), persistent=False)
            self.register_buffer('efeats', prep(efeats), persistent=False)
        else:
            # --no_feat_buffer (feature_getter.py:41-47,86-87: tables stay on the CPU, rows are copied per lookup): here the
            # tables stay in PINNED host memory, which the GPU addresses directly - the kernels read the rows they need over
            # the host link, nothing is staged and `.to(device)` does not move them (plain attributes, as in the reference)
            pin = lambda t: None if t is None else (t.pin_memory() if torch.cuda.is_available() else t)
            self.nfeats, self.efeats = pin(prep(nfeats)), pin(prep(efeats))
        self.nfeat_dim = nd if nd else dim
        self.efeat_dim = ed if ed else dim

    def nfeats_all_zero(self) -> bool:
        """True when there is no node-feature table or every entry of it is zero (every JODIE data set).  Checked once per
        table version (one reduction); consumers may then skip the table's column blocks (tg_seq_restarter.nfeats_zero)."""
        t = self.nfeats
        if t is None:
            return True
        key = (t.data_ptr(), t._version, tuple(t.shape))
        hit = getattr(self, '_nz_cache', None)
        if hit is None or hit[0] != key:
            hit = (key, not bool(torch.count_nonzero(t).item()))
            self._nz_cache = hit
        return hit[1]

    def append_node_rows(self, rows, reserve: Optional[int] = None) -> bool:
        """Append rows to the node table (online admission of new node ids, TIGE.grow_nodes): `rows` [k, d_n], or an int k
        for k zero rows -> whether the table's data pointer moved.  As `append_edge_rows`: the table is the leading view
        of a backing store that grows by half (reserve=: rows of a new store, as Memory.grow), `n_nodes` follows.  Refused, with nothing changed: a getter without a node
        table (n_nodes comes from it: NotImplementedError), a table in pinned host memory (register_buffer=False:
        NotImplementedError), rows of another width, a negative count or a reserve below the new row count (ValueError)."""
        from .memory import grow_capacity, grow_table
        if self.nfeats is None:
            raise NotImplementedError('append_node_rows: the feature getter has no node table (n_nodes is its row count)')
        if not self.pin_mem:
            raise NotImplementedError('append_node_rows: the node table lives in pinned host memory (register_buffer=False)')
        cur = self.nfeats
        if isinstance(rows, int):
            if rows < 0:
                raise ValueError(f'append_node_rows: {rows} rows')
            k, rows = rows, None
        else:
            rows = torch.as_tensor(rows)
            if rows.dim() != 2 or rows.shape[1] != cur.shape[1]:
                raise ValueError(f'append_node_rows: rows {tuple(rows.shape)} for a node table of width {cur.shape[1]}')
            k = rows.shape[0]
        n0 = cur.shape[0]
        moved = grow_table(self, 'nfeats', n0 + k, grow_capacity(n0, n0 + k, reserve))
        if rows is not None and k:
            self.nfeats[n0:] = rows.to(cur.device, cur.dtype)
        self.n_nodes = n0 + k
        self._version_ = getattr(self, '_version_', 0) + 1
        return moved

    def compact_node_rows(self, old_of, reserve: Optional[int] = None):
        """Keep the node-table rows of the ids old_of (int32, ascending: NodeCompaction.old_of), renumbered densely
        (TIGE.compact_nodes; Memory.compact: the same contract).  The table becomes the leading view of a NEW zeroed
        backing store, `n_nodes` follows.  Refused, with nothing changed: what `append_node_rows` refuses."""
        self._adopt_compacted(self._compact_build(old_of, reserve))

    def _compact_build(self, old_of, reserve):
        from .memory import compact_tables
        if self.nfeats is None:
            raise NotImplementedError('compact_node_rows: the feature getter has no node table (n_nodes is its row count)')
        if not self.pin_mem:
            raise NotImplementedError('compact_node_rows: the node table lives in pinned host memory (register_buffer=False)')
        cur = self.nfeats
        if not (torch.is_tensor(old_of) and old_of.dtype == torch.int32 and old_of.dim() == 1 and old_of.is_contiguous()
                and old_of.device == cur.device and 1 <= old_of.numel() <= cur.shape[0]):
            raise ValueError(f'compact_node_rows: old_of must be a contiguous 1-d int32 tensor of 1 to {cur.shape[0]} old ids '
                             f'on {cur.device}')
        return compact_tables([(self, 'nfeats')], old_of, reserve)

    def _adopt_compacted(self, built):
        from .memory import adopt_tables
        adopt_tables(built)
        self.n_nodes = built[0][3]
        self._version_ = getattr(self, '_version_', 0) + 1

    def set_node_rows(self, ids, rows, check: bool = True):
        """Overwrite rows of the node table (a dense id that is handed out again, TIGE.erase_keys / observe_keys): ids [k]
        int32 / int64, DISTINCT; `rows` [k, d_n], or the int 0 for zero rows.  The table's address does not move.  A model
        that derives tables from the node table (eager updates, query rows) is told by TIGE.set_node_rows.  Refused, with
        nothing changed: what `append_node_rows` refuses (no node table, a table in pinned host memory:
        NotImplementedError; rows of another shape: ValueError), ids that are no 1-d integer tensor, an int other than 0,
        an id outside [0, n_nodes) (ValueError; one read-back, check=False for ids the caller made itself)."""
        if self.nfeats is None:
            raise NotImplementedError('set_node_rows: the feature getter has no node table (n_nodes is its row count)')
        if not self.pin_mem:
            raise NotImplementedError('set_node_rows: the node table lives in pinned host memory (register_buffer=False)')
        cur = self.nfeats
        ids = torch.as_tensor(ids)
        if ids.dtype not in (torch.int32, torch.int64) or ids.dim() != 1:
            raise ValueError('set_node_rows: ids must be a 1-d int32 or int64 tensor')
        k = ids.numel()
        if isinstance(rows, int):
            if rows != 0:
                raise ValueError(f'set_node_rows: rows = {rows} (a tensor of rows, or 0 for zero rows)')
            rows = None
        else:
            rows = torch.as_tensor(rows)
            if rows.dim() != 2 or rows.shape[0] != k or rows.shape[1] != cur.shape[1]:
                raise ValueError(f'set_node_rows: rows {tuple(rows.shape)} for {k} ids of a node table of width {cur.shape[1]}')
        ids = ids.to(cur.device).long()
        if check and k and bool(((ids < 0) | (ids >= cur.shape[0])).any()):
            raise ValueError(f'set_node_rows: an id outside [0, {cur.shape[0]})')
        if k and rows is None:
            cur.index_fill_(0, ids, 0)
        elif k:
            cur.index_copy_(0, ids, rows.to(cur.device, cur.dtype))
        self._version_ = getattr(self, '_version_', 0) + 1

    def append_edge_rows(self, rows) -> bool:
        """Append rows [n, d_e] to the edge table (online ingestion, TIGE.observe) -> whether the table's data pointer moved
        (the caller then drops whatever caches it: TIGE.invalidate_struct).  The table is a leading view of a backing
        storage that grows geometrically, so most calls copy the new rows and nothing else.  Without an edge table there is
        nothing to do; tables pinned in host memory (register_buffer=False) do not grow."""
        if self.efeats is None:
            return False
        if not self.pin_mem:
            raise NotImplementedError('append_edge_rows: the edge table lives in pinned host memory (register_buffer=False)')
        cur = self.efeats
        rows = torch.as_tensor(rows).to(cur.device, cur.dtype).reshape(-1, cur.shape[1])
        n0, n1 = cur.shape[0], cur.shape[0] + rows.shape[0]
        store = getattr(self, '_ef_store', None)
        if (store is None or store.device != cur.device or store.data_ptr() != cur.data_ptr() or store.shape[0] < n0
                or store.shape[0] < n1):  # no backing yet (or the table was moved / replaced), or it is full: a new one
            store = torch.empty(max(n1, 2 * n0, 16), cur.shape[1], dtype=cur.dtype, device=cur.device)
            store[:n0] = cur
            self._ef_store = store
        store[n0:n1] = rows
        self.efeats = store[:n1]
        self.n_edges = n1
        return self.efeats.data_ptr() != cur.data_ptr()

    def compact_edge_rows(self, graph, keep_from: Optional[int] = None, pin=None, *, slack: Optional[int] = None,
                          swap: bool = True) -> Optional['EdgeRowsRelease']:
        """Release the rows of the edge table that `graph` no longer names (tg_edge_rows_*): the live rows - row 0, every
        row an entry of `graph` names, rows >= keep_from (default: none; rows of events not observed yet), the ids of
        `pin` - are packed in their old order into a NEW table -> EdgeRowsRelease(remap, eid_out, rows_before, rows,
        shift), or None without an edge table (nothing to do).  `eid_out` is what `graph.renumbered(remap, eid_out)`
        takes: the CALLER swaps the graph.  The new backing store has n_live + max(16, n_live // 4) rows (slack=: that many
        spare rows instead) and `efeats` is its leading n_live-row view, so the next `append_edge_rows` copies the new rows
        and nothing else.  Old and new table exist side by side until the old one is dropped (no in-place compaction).
        A device table is packed on the device (plan, ONE int64 read back, allocate, apply), a CPU table by the host twin.
        swap=False leaves this object as it was; `adopt_edge_rows(result)` swaps later (TIGE.release_edge_rows: graph and
        table change together).  Nothing has changed if it raises: NotImplementedError for a table in pinned host memory
        (register_buffer=False), ValueError for a bad keep_from / slack or an entry or pin that names no row."""
        if self.efeats is None:
            return None
        if not self.pin_mem:
            raise NotImplementedError('compact_edge_rows: the edge table lives in pinned host memory (register_buffer=False)')
        cur = self.efeats
        n_rows, d_e = cur.shape
        if slack is not None and int(slack) < 0:
            raise ValueError(f'compact_edge_rows: slack = {slack} is negative')
        spare = lambda n: max(16, n // 4) if slack is None else int(slack)
        if cur.device.type == 'cpu':
            remap, packed, eid_out = hip_ops.edge_rows_host(graph, cur.numpy(), n_rows, keep_from, pin)
            n_live = packed.shape[0]
            store = torch.empty(n_live + spare(n_live), d_e, dtype=cur.dtype)
            store[:n_live] = torch.from_numpy(packed)
            remap = torch.from_numpy(remap)
        else:
            remap, n_live, ws = hip_ops.edge_rows_plan(graph, n_rows, keep_from, pin, device=cur.device)
            store = torch.empty(n_live + spare(n_live), d_e, dtype=cur.dtype, device=cur.device)
            _, eid_out = hip_ops.edge_rows_apply(graph, cur, remap, n_live, ws, table_out=store)
        res = EdgeRowsRelease(remap, eid_out, n_rows, n_live, store)
        if swap:
            self.adopt_edge_rows(res)
        return res

    def adopt_edge_rows(self, res: 'EdgeRowsRelease'):
        """swap in the packed table of a `compact_edge_rows(..., swap=False)`"""
        self._ef_store = res._store
        self.efeats = res._store[:res.rows]
        self.n_edges = res.rows

    def install_rows(self, nfeats: Optional[Tensor] = None, efeats: Optional[Tensor] = None) -> bool:
        """Replace the node and / or the edge table by the given rows (TIGE.load_online: the tables of a saved online model)
        -> whether a table's data pointer moved (it does: the caller drops whatever caches it, TIGE.invalidate_struct).
        Each new table is the leading view of a backing store with the usual head-room - a zeroed one that is half as large
        again for the node table (`append_node_rows`), n + max(16, n // 4) rows for the edge table (`compact_edge_rows`) -
        so the next append copies the new rows and nothing else; `n_nodes` / `n_edges` follow.  None leaves a table as it
        is.  Refused, with nothing changed: a table the getter does not have, rows of another width or dtype (ValueError),
        tables in pinned host memory (register_buffer=False: NotImplementedError)."""
        from .memory import grow_capacity
        if not self.pin_mem:
            raise NotImplementedError('install_rows: the tables live in pinned host memory (register_buffer=False)')
        for name, new in (('nfeats', nfeats), ('efeats', efeats)):
            cur = getattr(self, name)
            if new is None:
                continue
            if cur is None:
                raise ValueError(f'install_rows: the feature getter has no {name} table')
            if not torch.is_tensor(new) or new.dim() != 2 or new.shape[1] != cur.shape[1] or new.dtype != cur.dtype:
                what = f'{new.dtype} {tuple(new.shape)}' if torch.is_tensor(new) else type(new).__name__
                raise ValueError(f'install_rows: {name} {what} for a {cur.dtype} table of width {cur.shape[1]}')
        moved = False
        if nfeats is not None:
            cur, n = self.nfeats, nfeats.shape[0]
            store = torch.zeros(grow_capacity(n, n, None), cur.shape[1], dtype=cur.dtype, device=cur.device)
            store[:n] = nfeats.to(cur.device)
            self.__dict__.setdefault('_stores', {})['nfeats'] = store
            self.nfeats = store[:n]
            self.n_nodes = n
            self._version_ = getattr(self, '_version_', 0) + 1
            self._nz_cache = None  # (keyed by the table's address: a freed store's address can come back)
            moved = True
        if efeats is not None:
            cur, n = self.efeats, efeats.shape[0]
            store = torch.empty(n + max(16, n // 4), cur.shape[1], dtype=cur.dtype, device=cur.device)
            store[:n] = efeats.to(cur.device)
            self._ef_store = store
            self.efeats = store[:n]
            self.n_edges = n
            moved = True
        return moved

    def _lookup(self, table, ids, width):
        if table is None:
            return torch.zeros(*ids.shape, width, device=ids.device)
        return hip_ops.gather_rows(table, ids)  # a pinned host table is read in place by the kernel

    def get_node_embeddings(self, nids: Tensor) -> Tensor:
        return self._lookup(self.nfeats, nids, self.out_dim)

    def get_edge_embeddings(self, eids: Tensor) -> Tensor:
        return self._lookup(self.efeats, eids, self.out_dim)
