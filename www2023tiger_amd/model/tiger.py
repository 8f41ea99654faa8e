"""Mirror of tiger/model/tiger.py: `TIGE` / `TIGER` with the reference's constructor,
method names, buffer/parameter names (state_dict compatible, alias keys included),
executed by libtiger_hip.so.

Ways to run a batch:
  * `contrast_learning(src, dst, neg, ts, eids, computation_graph)` - the reference
    signature.  In train() mode with autograd on, the whole iteration (collate, STEP 1-7,
    backward, write-back; `contrast_and_mutual_learning` adds the mutual loss) is one
    tg_train_step and the returned losses carry an autograd node that hands the finished
    gradients to the parameters.  In eval() / no_grad mode the batch is one tg_train_step
    without gradient buffers; where that call does not apply (non-default sampling strategy,
    a foreign ComputationGraph) STEP 1-6 run as one HIP entry point per reference method
    and STEP 7 in torch.
  * `stream_step(src, dst, neg, ts64, eids)` - collation and STEP 1-6 fused behind one
    C call (tg_stream_step) with no host synchronisation; the benchmarked path.
  * `fuse_attention()` - inference with fixed parameters: pre-multiplied attention weights.
"""
import ctypes as C
import operator
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np
import os
import weakref

import torch
from torch import Tensor, nn

from .. import hip_ops
from .._lib import TG_FORM_FC2_DEFERRED, TG_INVOLVED_MAX_K, TG_TOPK_MAX_K, TgLazyRestart, TgLinear, TgModel, TgStepIo, check, lib, ptr
from ..hip_ops import stream_ptr
from .basic_modules import MergeLayer
from .memory import Memory, MessageStoreNoGradLastOnly
from .message_modules import (IdentityMessageFunction, LastMessageAggregatorNoGradLastOnly, LinearMessageFunction,
                              MLPMessageFunction)
from .temporal_agg_modules import GraphAttnEmbedding
from .time_encoding import TimeEncode
from .update_modules import GRUUpdater, MergeUpdater
from .utils import select_latest_nids

_TSFM = {'id': 0, 'linear': 1, 'mlp': 2}
_UPD = {'gru': 0, 'merge': 1}


class EventAdmission(NamedTuple):
    """What `TIGE.observe_events` did with a batch.  eids int32 [n]: the edge row of every delivered event - a new row for
    a kept one, the row of its first copy for a duplicate; keep int64 [n_kept]: the positions that were observed,
    ascending (the first occurrences of the keys not seen before); n_kept = len(keep)."""
    eids: Tensor
    keep: Tensor
    n_kept: int


class _QueryGraph:
    """What the embedding reads of a computation graph (layers, involved bitmap), for a flat list of (node, t) queries"""

    def __init__(self, layers, bitmap):
        self.layers, self.bitmap = layers, bitmap


class CatalogueSnapshot:
    """A shared catalogue embedded ONCE at one time t (TIGE.embed_catalogue), for TIGE.recommend in place of `cand`:
    ids int64 [C], h float32 [C, d] (the items' embeddings at t), nb int64 [C, K] (their recent-edges neighbour ids at t,
    None for hit_type 'none') and t.  It remembers what it is a function of - the model, its device, the graph's node
    count and serial number, and the model's state / step / attention-parameter stamps at the time of embedding - so
    that recommend can refuse a snapshot that no longer describes the model.  P float32 [C, d], the items' half of the
    score head's first layer (tg_rank_cand_half), is computed on first use and again whenever the score head's
    parameters have changed since.  col_of int32 [n_nodes], the row of every node id in the snapshot and -1 for a node
    that is not in it (`hip_ops.catalogue_index(ids, n_nodes)`), is built on first use - recommend_subset gathers
    through it - and raises ValueError for a snapshot that lists an id twice.  A snapshot is read-only: nothing in it is
    updated by later calls.  A snapshot is either uniform in time (t_row is None: every row at t) or carries t_row float64
    [C], the time each row was embedded at (TIGE.refresh_catalogue: rows no change reached keep their bits and their
    time; t is then the time of the latest refresh).  change_epoch: the epoch of the model's ChangeTracker when the rows
    were computed (None without tracking) - a snapshot is refreshable while it equals the tracker's."""

    def __init__(self, model, ids: Tensor, h: Tensor, nb: Optional[Tensor], t: float, graph, stamp):
        self._model = weakref.ref(model)
        self.ids, self.h, self.nb, self.t = ids, h, nb, float(t)
        self.device = ids.device
        self.n_nodes = int(graph.num_node)
        self.graph_serial = getattr(graph, 'serial', None)
        self.stamp = stamp
        self._P = None
        self._P_stamp = None
        self._col_of = None
        self._inv_norm = None
        self.t_row = None
        self.change_epoch = None

    @property
    def model(self):
        return self._model()

    @property
    def col_of(self) -> Tensor:
        if self._col_of is None:
            self._col_of = hip_ops.catalogue_index(self.ids, self.n_nodes)
        m = self.model
        grown = int(getattr(m, 'n_nodes', 0) or 0) - int(self._col_of.numel())
        if grown > 0:  # the model admitted node ids since (TIGE.grow_nodes): none of them is in the snapshot
            self._col_of = torch.cat([self._col_of, self._col_of.new_full((grown,), -1)])
        return self._col_of

    @property
    def inv_norm(self) -> Tensor:
        """float32 [C]: 1 / ||h[j]||, the norm taken in float64 and the reciprocal rounded once; 0 for a zero or non-finite
        norm.  Built on first use (TIGE.similar_items with metric='cos' passes it to tg_knn_rows on both sides) and kept:
        h is read-only.  A refreshed snapshot is a new object and computes its own."""
        if self._inv_norm is None:
            n = self.h.double().pow(2).sum(1).sqrt()
            ok = torch.isfinite(n) & (n > 0)
            self._inv_norm = torch.where(ok, 1.0 / torch.where(ok, n, torch.ones_like(n)), torch.zeros_like(n)).float()
        return self._inv_norm

    def __len__(self):
        return int(self.ids.numel())


class ChangeTracker:
    """What changed under the rows of a catalogue snapshot (TIGE.track_changes, TIGE.refresh_catalogue).
    bits: a `hip_ops.new_bitmap` over the model's node ids - every node whose per-node state row (memories, mailbox,
    node-feature row) or T-CSR row changed since `clear()`; whole: everything may have changed (`reason` says why);
    epoch: bumped by `clear()` - a snapshot whose change_epoch equals it has seen every change the bits hold.  The model's
    own writers mark what they write; writes through raw tensors by third parties are the caller's to `mark`."""

    def __init__(self, n_nodes: int, device):
        self.n_nodes = int(n_nodes)
        self.bits = hip_ops.new_bitmap(self.n_nodes, device)
        self.whole, self.reason, self.epoch = False, None, 0

    def fit(self, n_nodes: int):
        """the model admitted node ids (grow_nodes): the bitmap follows"""
        if n_nodes > self.n_nodes:
            self.bits = hip_ops.bitmap_grown(self.bits, n_nodes)
            self.n_nodes = int(n_nodes)

    def mark(self, ids):
        ids = torch.as_tensor(ids).to(self.bits.device).long().reshape(-1)
        if ids.numel() and not self.whole:
            hip_ops.bitmap_mark(ids, self.bits, self.n_nodes)

    def mark_graph(self, old, new):
        """every node whose T-CSR row length differs between the two graphs (tg_bitmap_mark_degree_diff): exact for
        children that only add or only remove entries (extended, merged, trimmed, without); nothing for `renumbered`,
        which shares indptr.  A graph without device arrays: mark_all."""
        if old is new or self.whole:
            return
        if old is None or new is None or getattr(old, '_dev', None) is None or getattr(new, '_dev', None) is None:
            return self.mark_all('a graph without device arrays was swapped in or out')
        self.fit(max(old.num_node, new.num_node))
        if old._dev[0] is not new._dev[0]:
            hip_ops.bitmap_mark_degree_diff(old, new, self.bits)

    def mark_all(self, reason: str):
        if not self.whole:
            self.whole, self.reason = True, reason

    def clear(self):
        self.bits.zero_()
        self.whole, self.reason = False, None
        self.epoch += 1

    def renumbered(self, n_nodes: int):
        """the node ids were renumbered (compact_nodes): a fresh bitmap over the new ids, a new epoch, everything changed"""
        self.n_nodes = int(n_nodes)
        self.bits = hip_ops.new_bitmap(self.n_nodes, self.bits.device)
        self.epoch += 1
        self.whole, self.reason = True, 'compact_nodes / compact_keys renumbered the node ids'


class OnlineJournal:
    """What changed since the last saved online state file, and the writer of the next one (TIGE.journal,
    TIGE.apply_online_delta).  A sink of the model's writers beside the ChangeTracker and independent of it:
    both may be installed, clearing one loses nothing for the other.  Two bitmaps over the node ids - state_bits: the
    per-node state row (both memories, mailbox, node-feature row) changed; graph_bits: the T-CSR row changed - so a restart
    does not drag T-CSR rows into a file.  whole: the next file must be a base (`reason` says why): everything that sets a
    tracker's `whole`, and a graph whose eids were renumbered (`release_edge_rows` shares indptr with its parent: no
    degree changes).  As of the last save: chain (the id of the base the files follow), seq (0: the base), and the counts a
    delta states as its "before": edge-table rows, n_nodes, the graph's nodes and entries.
    REPLAYS OF A CAPTURED DEVICE GRAPH ARE INVISIBLE, exactly as for the tracker: whoever replays captured steps between
    two saves calls `mark(ids)` / `mark_all(...)` itself, as for writes through raw tensors.
    NOT in a delta: parameters (deltas are for eval() mode), optimiser state, `uptodate` bitmaps, snapshots, held eids.
    A dirty T-CSR row is saved WHOLE: a hub row costs its full length per delta unless `forget(keep_last=M)` bounds it.
    Keeping the files in order and durable is the caller's job."""
    DELTA_FORMAT, DELTA_VERSION = 'tiger-online-delta', 1

    def __init__(self, model):
        self._model = weakref.ref(model)
        self.n_nodes = int(model.n_nodes)
        dev = model.device
        self.state_bits = hip_ops.new_bitmap(self.n_nodes, dev)
        self.graph_bits = hip_ops.new_bitmap(self.n_nodes, dev)
        self.whole, self.reason = True, 'no base has been saved on this chain yet'
        self.chain, self.seq, self.saved = None, -1, None

    @property
    def model(self):
        return self._model()

    # ---- the sink the model's writers feed (the interface of ChangeTracker) ------------------------------------------
    def fit(self, n_nodes: int):
        if n_nodes > self.n_nodes:
            self.state_bits = hip_ops.bitmap_grown(self.state_bits, n_nodes)
            self.graph_bits = hip_ops.bitmap_grown(self.graph_bits, n_nodes)
            self.n_nodes = int(n_nodes)

    def admitted(self, n0: int, n1: int):
        """a growth that gave the ids [n0, n1) feature rows: their state rows are no longer those of a grown table"""
        self.fit(n1)
        if n1 > n0:
            self.mark(torch.arange(n0, n1, device=self.state_bits.device))

    def mark(self, ids):
        ids = torch.as_tensor(ids).to(self.state_bits.device).long().reshape(-1)
        if ids.numel() and not self.whole:
            hip_ops.bitmap_mark(ids, self.state_bits, self.n_nodes)

    def mark_graph(self, old, new):
        if old is new or self.whole:
            return
        if old is None or new is None or getattr(old, '_dev', None) is None or getattr(new, '_dev', None) is None:
            return self.mark_all('a graph without device arrays was swapped in or out')
        self.fit(max(old.num_node, new.num_node))
        if old._dev[0] is not new._dev[0]:
            hip_ops.bitmap_mark_degree_diff(old, new, self.graph_bits)
        elif any(a is not b for a, b in zip(old._dev, new._dev)):
            self.mark_all('the graph was renumbered: every edge id (or neighbour) changed under unchanged row bounds')

    def mark_all(self, reason: str):
        if not self.whole:
            self.whole, self.reason = True, reason

    def renumbered(self, n_nodes: int):
        self.n_nodes = int(n_nodes)
        self.state_bits = hip_ops.new_bitmap(self.n_nodes, self.state_bits.device)
        self.graph_bits = hip_ops.new_bitmap(self.n_nodes, self.state_bits.device)
        self.whole, self.reason = True, 'compact_nodes / compact_keys renumbered the node ids'

    # ---- files ------------------------------------------------------------------------------------------------------
    def _position(self, chain: int, seq: int):
        """the model IS the state of file `seq` of `chain`: nothing is dirty"""
        m = self.model
        self.fit(m.n_nodes)
        self.state_bits.zero_()
        self.graph_bits.zero_()
        self.whole, self.reason = False, None
        self.chain, self.seq = int(chain), int(seq)
        fg, g = m.raw_feat_getter, m.graph
        entries = int(g.tcsr.num_entry) if m.device.type == 'cuda' else len(g._host_tcsr()[1])  # (a host model: bases only)
        self.saved = dict(efeat_rows=0 if fg.efeats is None else int(fg.efeats.shape[0]), n_nodes=int(m.n_nodes),
                          graph_nodes=int(g.num_node), num_entry=entries)

    @staticmethod
    def per_node_tables(m):
        """name -> the per-node tensors a delta carries rows of (the two REAL memories, not the alias modules), in the order
        they are gathered; the mailbox's has-message bit travels as one byte per id beside them"""
        L, R, S, fg = m.left_memory, m.right_memory, m.msg_store, m.raw_feat_getter
        out = {f'{side}.{name}': getattr(mem, name) for side, mem in (('left', L), ('right', R)) for name in mem.COMPACT_TABLES}
        out.update(node_msg_vals=S.node_msg_vals, node_msg_ts=S.node_msg_ts)
        if fg.nfeats is not None:
            out['nfeats'] = fg.nfeats
        return out

    def _refusals(self, what: str):
        m = self.model
        if m is None:
            raise RuntimeError(f'{what}: the model of this journal is gone')
        if m._journal is not self:
            raise RuntimeError(f'{what}: this journal is no longer the model\'s (load_online installed another)')
        m._refuse_partitioned(what)
        if m.training:
            raise RuntimeError(f'{what}: online state files are written in eval() mode (the streaming state of a served model)')
        if not m.raw_feat_getter.pin_mem:
            raise NotImplementedError(f'{what}: the feature tables live in pinned host memory (register_buffer=False)')
        if m.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{what}: a state file cannot be written while a stream is being captured into a graph')
        return m

    @torch.no_grad()
    def save(self, f) -> str:
        """Write the next file of the chain to `f` (a path or a file object) -> 'base' or 'delta'.  The first save, and any
        save after `whole` was set, is a BASE: `online_state()` plus `chain` (a new id) and `seq` = 0 - a file `load_online`
        reads as any other.  Every other save is a DELTA (format 'tiger-online-delta', one `torch.save` dict, loadable with
        weights_only=True): the rows of the ids of state_bits from every per-node tensor, the edge-table rows appended
        since the last save, the T-CSR rows of graph_bits packed (tg_tcsr_rows_pack), the graph's small state whole, and
        the counts before and after.  Device work of a delta: two bitmap listings, two row gathers (8 + 1 tables), one bit
        gather, the pack's plan and copy; two read-backs (both list counts together; the packed length) besides the copies
        of the payload.  Afterwards both bitmaps are clear and seq has advanced; if the save raises, the journal is
        unchanged.  Refused: what `save_online` / `load_online` refuse (training mode, a partitioned model, tables in pinned
        host memory, a stream capture in progress)."""
        m = self._refusals('OnlineJournal.save')
        m._poll_train_errors()
        if self.whole or self.chain is None:
            chain = int.from_bytes(os.urandom(8), 'little') >> 1
            st = m.online_state()
            st.update(chain=chain, seq=0)
            torch.save(st, f)
            self._position(chain, 0)
            return 'base'
        if m.device.type != 'cuda':
            raise RuntimeError(f'OnlineJournal.save: the model lives on {m.device}; deltas are cut on the GPU')
        st = self._delta(m)
        torch.save(st, f)
        self._position(self.chain, self.seq + 1)
        return 'delta'

    def _listed(self, m):
        """the set bits of both bitmaps as ascending int32 lists: two listings, ONE read-back of both counts"""
        n = int(m.n_nodes)
        self.fit(n)
        a, b = hip_ops.unique_compact(self.state_bits, n, n), hip_ops.unique_compact(self.graph_bits, n, n)
        ca, cb = torch.stack([a['count'][0], b['count'][0]]).tolist()
        return a['ids'][:ca].int(), b['ids'][:cb].int()

    def _delta(self, m) -> dict:
        fg, S, g, dev = m.raw_feat_getter, m.msg_store, m.graph, m.device
        g.tcsr  # (a graph that was never sampled from has no device arrays yet)
        ids, rows = self._listed(m)
        D = int(ids.numel())
        cpu = lambda t: t.detach().to('cpu', copy=True)
        packed = {}
        tables = self.per_node_tables(m)
        if D:
            for name, t in tables.items():
                row_bytes = t.element_size() * int(np.prod(t.shape[1:], dtype=np.int64))
                if row_bytes not in (1, 4, 8) and row_bytes % 16:
                    raise NotImplementedError(f'OnlineJournal.save: rows of {row_bytes} bytes ({name}) are not gathered '
                                              '(a multiple of 16, or 8, 4 or 1)')
            pairs = [(t, torch.empty((D,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)) for t in tables.values()]
            for i in range(0, len(pairs), hip_ops._lib.TG_NODE_ROWS_MAX):  # (as few launches as the table limit allows)
                hip_ops.node_rows_compact(pairs[i:i + hip_ops._lib.TG_NODE_ROWS_MAX], ids)
            words = hip_ops.bitmap_compact(S.has_msg_bits, ids, int(m.n_nodes), D)
            j = torch.arange(D, device=dev)
            has = ((words[j >> 6] >> (j & 63)) & 1).to(torch.uint8)
            packed = {name: cpu(dst) for name, (_, dst) in zip(tables, pairs)}
        else:
            packed = {name: torch.empty((0,) + tuple(t.shape[1:]), dtype=t.dtype) for name, t in tables.items()}
            has = torch.empty(0, dtype=torch.uint8)
        off, ts, nbr, eid = hip_ops.tcsr_rows_pack(g, rows)
        before = self.saved
        rows_now = 0 if fg.efeats is None else int(fg.efeats.shape[0])
        if rows_now < before['efeat_rows'] or m.n_nodes < before['n_nodes'] or g.num_node < before['graph_nodes']:
            raise RuntimeError('OnlineJournal.save: a table or the graph shrank and nothing told the journal (mark_all)')
        kind, key, pos, has_gauss, gauss = g.rng.get_state()
        return dict(
            format=self.DELTA_FORMAT, version=self.DELTA_VERSION, chain=int(self.chain), seq=int(self.seq) + 1,
            fingerprint=m._online_fingerprint(),
            n_nodes_before=before['n_nodes'], n_nodes_after=int(m.n_nodes),
            graph_nodes_before=before['graph_nodes'], graph_nodes_after=int(g.num_node),
            num_entry_before=before['num_entry'], num_entry_after=int(g.tcsr.num_entry),
            efeat_rows_before=before['efeat_rows'], efeat_rows_after=rows_now,
            ids=cpu(ids), rows_of=packed, has_msg=cpu(has),
            efeats_tail=None if fg.efeats is None else cpu(fg.efeats[before['efeat_rows']:rows_now]),
            rows=cpu(rows), off=cpu(off), ts=cpu(ts), nbr=cpu(nbr), eid=cpu(eid),
            graph_state=dict(t_last=float(g._t_last), time_ordered=bool(g._time_ordered), rng_kind=str(kind),
                             rng_key=torch.from_numpy(key.astype(np.int64)), rng_pos=int(pos), rng_has_gauss=int(has_gauss),
                             rng_cached_gaussian=float(gauss),
                             mt_state=None if g._mt is None else g._mt.detach().to('cpu', copy=True)))


class TIGE(nn.Module):
    _born_rows = None
    _tracker = None          # ChangeTracker (track_changes), None: nothing is recorded
    _journal = None          # OnlineJournal (journal), None: nothing is recorded
    last_refreshed = None    # (n_dirty, n_by_age) of the latest refresh_catalogue

    @staticmethod
    def born_with_rows(n_rows: int):
        """Context: models constructed inside allocate `n_rows` rows per state table instead of one per node - a rank of the
        physically partitioned multi-GPU layout, whose engine installs the node -> row map right after (dist.py:
        HipPartitionEngine.partition).  Until then such a model must not run."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            prev, TIGE._born_rows = TIGE._born_rows, int(n_rows)
            try:
                yield
            finally:
                TIGE._born_rows = prev
        return ctx()

    def __init__(self, *, raw_feat_getter, graph, n_neighbors: int = 20, n_layers: int = 2, n_head: int = 2,
                 dropout: float = 0.1, msg_src: str, upd_src: str, msg_tsfm_type: str = 'id',
                 mem_update_type: str = 'gru', tgn_mode: bool = True, msg_last_only: bool = True,
                 hit_type: str = 'none'):
        super().__init__()
        if not msg_last_only:
            raise NotImplementedError('only the last-message mailbox is built (init_utils.py:166)')
        self.raw_feat_getter = raw_feat_getter
        self.n_nodes = raw_feat_getter.n_nodes
        self.nfeat_dim = raw_feat_getter.nfeat_dim
        self.efeat_dim = raw_feat_getter.efeat_dim
        self.time_encoder = TimeEncode(dim=self.nfeat_dim)
        self.tfeat_dim = self.time_encoder.dim
        self.memory_dim = self.nfeat_dim
        self.raw_msg_dim = self.memory_dim * 2 + self.efeat_dim + self.tfeat_dim
        self.n_neighbors, self.n_layers, self.n_head = n_neighbors, n_layers, n_head
        self.msg_src, self.upd_src = msg_src, upd_src
        self.tgn_mode, self.msg_last_only = True, True
        self._sanity_check()

        rows = TIGE._born_rows if TIGE._born_rows is not None else self.n_nodes  # (born_with_rows: a partitioned rank)
        self.left_memory = Memory(rows, self.memory_dim)
        self.right_memory = Memory(rows, self.memory_dim)
        self.msg_store = MessageStoreNoGradLastOnly(rows, dim=self.raw_msg_dim)
        # module aliases: they appear as extra state_dict keys exactly as in the reference
        self.msg_memory = self.left_memory if msg_src == 'left' else self.right_memory
        self.upd_memory = self.left_memory if upd_src == 'left' else self.right_memory
        self.msg_aggregate_fn = LastMessageAggregatorNoGradLastOnly(raw_feat_getter=raw_feat_getter,
                                                                   time_encoder=self.time_encoder)
        fn = {'id': IdentityMessageFunction, 'linear': LinearMessageFunction, 'mlp': MLPMessageFunction}
        if msg_tsfm_type not in fn:
            raise NotImplementedError(msg_tsfm_type)
        self.msg_tsfm_type = msg_tsfm_type
        self.msg_transform_fn = fn[msg_tsfm_type](raw_msg_dim=self.raw_msg_dim)
        self.msg_dim = self.msg_transform_fn.output_size
        if mem_update_type == 'gru':
            self.right_mem_updater = GRUUpdater(self.msg_dim, self.memory_dim)
        elif mem_update_type == 'merge':
            self.right_mem_updater = MergeUpdater(self.msg_dim, self.memory_dim)
        else:
            raise NotImplementedError(mem_update_type)
        self.mem_update_type = mem_update_type
        self.temporal_embedding_fn = GraphAttnEmbedding(raw_feat_getter=raw_feat_getter,
                                                        time_encoder=self.time_encoder, graph=graph,
                                                        n_neighbors=n_neighbors, n_layers=n_layers, n_head=n_head,
                                                        dropout=dropout)
        self.hit_type = hit_type
        if hit_type == 'vec':
            merge_dim = self.nfeat_dim + self.n_neighbors
        elif hit_type == 'bin':
            self.hit_embedding = nn.Embedding(2, self.nfeat_dim)
            merge_dim = self.nfeat_dim
        elif hit_type == 'count':
            self.hit_embedding = nn.Embedding(self.n_neighbors + 1, self.nfeat_dim)
            merge_dim = self.nfeat_dim
        else:
            merge_dim = self.nfeat_dim
        self.score_fn = MergeLayer(merge_dim, merge_dim, self.nfeat_dim, 1, dropout=dropout)
        self.contrast_loss_fn = nn.BCEWithLogitsLoss()
        self._struct_cache = None
        self._fused = None
        self._pending = None        # eager updates: table of precomputed updater rows (see eager_updates)
        self._pending_stamp = None  # state stamp the table is current for
        self._state_version = 0     # bumped by every method that changes state outside the eager streaming step
        self._step_ws = {}

    def _sanity_check(self):
        if self.msg_src not in {'left', 'right'}:
            raise ValueError(f'Invalid msg_src={self.msg_src}')
        if self.upd_src not in {'left', 'right'}:
            raise ValueError(f'Invalid upd_src={self.upd_src}')

    # ---- plumbing ---------------------------------------------------------------------
    def restart_list(self, nids: Tensor, t_dev: Tensor):
        """`restart(nids, t.expand(n))` for a device-resident id list and ONE device-resident time, with the SeqRestarter
        (inference form, or train() mode with its dropout), as a single library call (tg_restart_seq_list(_train): histories, anonymised ids, the restarter's
        forward, the state update) - the loops that restart per batch (eval_utils: lazy restart) were bound by the host
        side of the dozen calls this replaces.  Anything else takes `restart`."""
        from .restarters import SeqRestarter
        r = self.restarter_fn
        n = int(nids.numel())
        # (whatever strategy the restarter's graph samples neighbourhoods with, histories are recent-edges lists: graph.py:150-155)
        if (n == 0 or not isinstance(r, SeqRestarter) or getattr(self, '_row_of', None) is not None
                or self.device.type != 'cuda' or t_dev.dtype != torch.float32):
            return self.restart(nids, t_dev.expand(n))
        p = float(r.mha_fn.dropout)
        train = r.training and p > 0
        if train and (r.rng_fn is None or float(r.merger.dropout.p) != p):
            return self.restart(nids, t_dev.expand(n))
        self._touch()
        self._mark(nids)
        m, rs = self.model_struct(), r._struct()
        nbytes = int(lib.tg_restart_seq_list_workspace_bytes(C.byref(m), C.byref(rs), n))
        ws = getattr(self, '_restart_list_ws', None)
        if ws is None or ws.numel() < nbytes:
            ws = self._restart_list_ws = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=self.device)
        if train:  # train() mode: attention / merger dropout is active, as when the reference restarts inside its training loop
            check(lib.tg_restart_seq_list_train(C.byref(m), C.byref(r.graph.tcsr), C.byref(rs), n, ptr(nids), ptr(t_dev), p,
                                                ptr(r.rng_fn()), ptr(ws), ws.numel(), stream_ptr(self.device)),
                  'tg_restart_seq_list_train')
            return
        check(lib.tg_restart_seq_list(C.byref(m), C.byref(r.graph.tcsr), C.byref(rs), n, ptr(nids), ptr(t_dev), ptr(ws),
                                      ws.numel(), stream_ptr(self.device)), 'tg_restart_seq_list')

    def restart_list_keep_tables(self, nids: Tensor, t_dev: Tensor):
        """`restart_list` on a model that may stream with eager updates: were its per-node tables current?  Then they
        follow the restart - the restarted nodes have no pending message any more and new memories: their centre / query
        rows are recomputed (`_tables_follow_restart`) - instead of being rebuilt for every node at the next step."""
        current = (self._pending is not None and self._pending_stamp == self._state_stamp()
                   and (getattr(self, '_gtab', None) is None or getattr(self, '_gtab_stamp', None) is not None))
        self.restart_list(nids, t_dev)  # (one library call for the SeqRestarter, TIGER.restart otherwise)
        if current:
            self._tables_follow_restart(nids)

    def restart_list_split_ok(self) -> bool:
        """Can `restart_list` be taken apart into `restart_list_forward` (reads graph / features / restarter parameters only)
        and `restart_list_apply` (the state update)?  The SeqRestarter in inference form."""
        from .restarters import SeqRestarter
        r = self.restarter_fn
        return (isinstance(r, SeqRestarter) and not (r.training and float(r.mha_fn.dropout) > 0)
                and getattr(self, '_row_of', None) is None and self.device.type == 'cuda')

    def restart_list_forward(self, nids: Tensor, t_dev: Tensor, h_left: Tensor, h_right: Tensor, prev_ts: Tensor, ws_key='a'):
        """The restarter's rows of `restart_list` WITHOUT the state update (tg_restart_seq_list_fwd), on the current stream,
        into the caller's buffers.  Nothing a streaming step writes is read: callable on a second stream beside a step."""
        r = self.restarter_fn
        n = int(nids.numel())
        m, rs = self.model_struct(), r._struct()
        nbytes = int(lib.tg_restart_seq_list_workspace_bytes(C.byref(m), C.byref(rs), n))
        store = self.__dict__.setdefault('_restart_fwd_ws', {})
        ws = store.get(ws_key)
        if ws is None or ws.numel() < nbytes:
            ws = store[ws_key] = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=self.device)
        check(lib.tg_restart_seq_list_fwd(C.byref(m), C.byref(r.graph.tcsr), C.byref(rs), n, ptr(nids), None, ptr(t_dev),
                                          ptr(h_left), ptr(h_right), ptr(prev_ts), ptr(ws), ws.numel(),
                                          stream_ptr(self.device)), 'tg_restart_seq_list_fwd')

    def restart_lists_forward(self, lists, t_devs):
        """`restart_list_forward` over several device-resident lists at once, each at its own device-resident time
        (tg_restart_seq_lists_fwd: one forward; at most 8 lists) -> (ids, h_left, h_right, prev_ts): the lists concatenated
        (empty ones skipped) and their rows.  The lists of consecutive batches of a restart loop are independent of each other."""
        r, dev, d = self.restarter_fn, self.device, self.memory_dim
        counts = [int(x.numel()) for x in lists]
        n = sum(counts)
        ids = torch.empty(n, dtype=torch.int64, device=dev)
        hl, hr, pt = torch.empty(n, d, device=dev), torch.empty(n, d, device=dev), torch.empty(n, device=dev)
        if n == 0:
            return ids, hl, hr, pt
        m, rs = self.model_struct(), r._struct()
        nbytes = int(lib.tg_restart_seq_list_workspace_bytes(C.byref(m), C.byref(rs), n))
        ws = torch.empty(nbytes + 1024, dtype=torch.uint8, device=dev)
        k = len(lists)
        lp = (C.c_void_p * k)(*[ptr(x) for x in lists])
        tp = (C.c_void_p * k)(*[ptr(t) for t in t_devs])
        cn = (C.c_int64 * k)(*counts)
        check(lib.tg_restart_seq_lists_fwd(C.byref(m), C.byref(r.graph.tcsr), C.byref(rs), k, lp, cn, tp, ptr(ids), ptr(hl), ptr(hr),
                                           ptr(pt), ptr(ws), ws.numel(), stream_ptr(dev)), 'tg_restart_seq_lists_fwd')
        return ids, hl, hr, pt

    def restart_list_apply(self, nids: Tensor, h_left: Tensor, h_right: Tensor, prev_ts: Tensor):
        """The state update of `restart_list` (tiger.py:603,608-609) from rows `restart_list_forward` left."""
        self._touch()
        self._mark(nids)
        m = self.model_struct()
        check(lib.tg_restart_apply(C.byref(m), int(nids.numel()), ptr(nids), ptr(h_left), ptr(h_right), ptr(prev_ts),
                                   stream_ptr(self.device)), 'tg_restart_apply')

    def restart_list_captured(self, nids_cap: Tensor, n_dev: Tensor, t_dev: Tensor):
        """The device half of `restart_list` + `_tables_follow_restart` with the live count ON THE DEVICE (n_dev, int32): launches
        sized for the capacity len(nids_cap), the first n_dev entries restarted (tg_restart_seq_list_dev, tg_attn_gtab_rows with
        its device count).  No host value depends on the count: callable under stream capture; the caller replays the graph
        for every batch whose count fits and does the host-side bookkeeping itself (eval_utils._RestartPipeline)."""
        r = self.restarter_fn
        cap = int(nids_cap.numel())
        self._mark_all('restart_list_captured: the count of restarted nodes lives on the device')
        m, rs = self.model_struct(), r._struct()
        nbytes = int(lib.tg_restart_seq_list_workspace_bytes(C.byref(m), C.byref(rs), cap))
        ws = getattr(self, '_restart_cap_ws', None)
        if ws is None or ws.numel() < nbytes:
            ws = self._restart_cap_ws = torch.empty(nbytes + 1024, dtype=torch.uint8, device=self.device)
        check(lib.tg_restart_seq_list_dev(C.byref(m), C.byref(r.graph.tcsr), C.byref(rs), cap, ptr(nids_cap), ptr(n_dev),
                                          ptr(t_dev), ptr(ws), ws.numel(), stream_ptr(self.device)), 'tg_restart_seq_list_dev')
        if self._pending is not None and getattr(self, '_gtab', None) is not None:
            ws2 = self._ws('gtab_rc', cap * (4 * self.memory_dim + 4) + 64)
            check(lib.tg_attn_gtab_rows(C.byref(m), cap, ptr(nids_cap), ptr(n_dev), ptr(ws2), ws2.numel(),
                                        stream_ptr(self.device)), 'tg_attn_gtab_rows(restart, captured)')

    @property
    def graph(self):
        return self.temporal_embedding_fn.graph

    @graph.setter
    def graph(self, new_obj):
        old = self.temporal_embedding_fn.graph
        self.temporal_embedding_fn.graph = new_obj
        for sink in self._sinks():
            sink.mark_graph(old, new_obj)

    # ---- change tracking ----------------------------------------------------
    def _sinks(self):
        """whoever records what the model's writers change: the snapshot tracker (track_changes), the journal (journal)"""
        return tuple(s for s in (self._tracker, self._journal) if s is not None)

    def journal(self) -> OnlineJournal:
        """-> the model's OnlineJournal (installed on first use): from now on the model's own writers record
        which nodes' state rows and which T-CSR rows change, and `journal().save(f)` writes a base file first and then
        deltas that hold only those rows (`load_online(base)` + `apply_online_delta(delta)`, in order, rebuild the model
        bit for bit).  Independent of `track_changes()`: both may be installed at once and neither clears the other.
        `load_online` of a base that carries chain / seq installs a journal positioned there."""
        if self._journal is None:
            self._journal = OnlineJournal(self)
        return self._journal
    def track_changes(self, enable: bool = True) -> Optional[ChangeTracker]:
        """Start (or, enable=False, stop) recording which nodes' state rows and T-CSR rows change -> the ChangeTracker
        (None when switched off).  Opt-in: nothing is recorded, and nothing costs anything, while it is off.  With a
        tracker installed the model's own writers mark what they write (a streaming step its src and dst, the graph
        setter the rows whose length changed, restarts / erase / set_node_rows / update_*_memory their ids; whatever
        rewrites everything - load_state_dict, reset, load_memory_state, flush_msg, load_online, compact_nodes, train(),
        a step with the in-step restart loop or over a resident stream - sets `whole`).  The evaluation and training
        steps of `contrast_learning` / `contrast_and_mutual_learning` mark as a streaming step does.  REPLAYS OF A CAPTURED
        DEVICE GRAPH ARE INVISIBLE to the tracker: the host runs no code when a graph is replayed, so a step captured
        before tracking was switched on marks nothing, and one captured with tracking on sets `whole` once, at capture
        time.  Whoever replays captured steps between two refreshes calls `tracker.mark_all(...)` (or `mark(ids)`)
        itself, as for writes through raw tensors.  Calling track_changes again while a tracker is installed returns
        that tracker."""
        if not enable:
            self._tracker = None
            return None
        if self._tracker is None:
            self._tracker = ChangeTracker(self.n_nodes, self.device)
        return self._tracker

    def _mark(self, ids):
        for sink in self._sinks():
            sink.mark(ids)

    def _mark_all(self, reason: str):
        for sink in self._sinks():
            sink.mark_all(reason)

    def _mark_step(self, buf, io):
        """what one step over the batch in `buf` writes (io: its tg_step_io), for launch_step and for the training /
        evaluation step of TrainBuffers.launch.  STEP 4-6 write the rows of the batch's positive nodes only (tg_memory.hip:
        one wavefront per unique positive node); the in-step restart loop re-initialises rows no host list names, a
        resident stream's batch is named by an offset on the device, and a step that is being captured into a device
        graph runs again at every replay, which the host does not see: those mark everything."""
        for tr in self._sinks():
            if io.lazy and getattr(buf, '_lazy_collate', None) is None:
                tr.mark_all('a step with the in-step lazy-restart loop')
            elif buf.offset is not None:
                tr.mark_all('a step over a resident stream: its batch offset lives on the device')
            elif self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                tr.mark_all('a step captured into a device graph: its replays are invisible to the host')
            else:
                tr.mark(buf.src)
                tr.mark(buf.dst)

    @property
    def device(self):
        return self.msg_memory.device

    def _apply(self, fn, *a, **kw):  # .to() / .cuda() move every tensor: pointers change
        eager, fused = self._pending is not None, self._fused is not None
        self._plists = None
        self._gtab = None
        self._ctab = None
        self._gtab_stamp = None
        self._struct_cache = None
        self._fused = None
        self._fused_l1 = None
        self._fc2_fold = None
        self._pending = None
        self._pending_stamp = None
        self._step_ws = {}
        out = super()._apply(fn, *a, **kw)
        if getattr(self, '_row_of', None) is not None:  # the row map of a partitioned model follows its tables
            self._row_of = fn(self._row_of)
        # derived tables follow the tensors to their new home: a model that streamed with eager updates / pre-multiplied
        # weights keeps doing so (silently falling back to the lazy forms would change nothing but the speed - and would
        # break engines that rely on the table, e.g. the partitioned multi-GPU layout)
        if eager:
            self.eager_updates()
        if fused and self.device.type == 'cuda':
            self.fuse_attention()
        return out

    def dropout_rng(self) -> Tensor:
        """device int64[2] = {seed, step counter} of the dropout mask generator (training only)"""
        t = self._step_ws.get('rng')
        if t is None or t.device != self.device:
            t = torch.tensor([torch.initial_seed() & (2 ** 63 - 1), 0], dtype=torch.int64, device=self.device)
            self._step_ws['rng'] = t
        return t

    def invalidate_struct(self):
        self._struct_cache = None

    def model_struct(self, layer: int = 0) -> TgModel:
        """tg_model view of this module's tensors (cached until tensors are re-homed).  layer: which attention layer's
        weights the struct carries (temporal_embedding_fn.fns[layer]; only the two-layer operator path asks for 1)."""
        if layer:
            base = self.model_struct()
            hit = getattr(self, '_struct_cache_l1', None)
            if hit is not None and hit[0] is base:
                return hit[1]
            m = TgModel.from_buffer_copy(base)  # ctypes structs with pointers do not copy.copy
            att = self.temporal_embedding_fn.fns[layer]
            lin = lambda l: TgLinear(ptr(l.weight), ptr(l.bias))
            mha = att.mha_fn
            m.attn_wq, m.attn_wk, m.attn_wv, m.attn_b_in = (ptr(mha.q_proj_weight), ptr(mha.k_proj_weight),
                                                           ptr(mha.v_proj_weight), ptr(mha.in_proj_bias))
            m.attn_out, m.attn_fc1, m.attn_fc2 = lin(mha.out_proj), lin(att.merger.fc1), lin(att.merger.fc2)
            f1 = getattr(self, '_fused_l1', None)
            m.attn_fused = ptr(f1) if f1 is not None else None
            self._struct_cache_l1 = (base, m)
            return m
        if self._struct_cache is not None:
            return self._struct_cache
        lin = lambda l: TgLinear(ptr(l.weight), ptr(l.bias))
        nul = TgLinear(None, None)
        fg, att = self.raw_feat_getter, self.temporal_embedding_fn.fns[0]
        for t in (fg.nfeats, fg.efeats):
            if t is not None and t.device != self.device and not (t.device.type == 'cpu' and t.is_pinned()):
                raise RuntimeError('feature tables must live on the model device or in pinned host memory '
                                   '(NumericalFeature(register_buffer=False) pins them)')
        tsfm1 = tsfm2 = nul
        if self.msg_tsfm_type == 'linear':
            tsfm1 = lin(self.msg_transform_fn.fn[1])
        elif self.msg_tsfm_type == 'mlp':
            tsfm1, tsfm2 = lin(self.msg_transform_fn.fn[1]), lin(self.msg_transform_fn.fn[4])
        gru = [None] * 4
        fc1 = fc2 = nul
        if self.mem_update_type == 'gru':
            c = self.right_mem_updater.cell
            gru = [ptr(c.weight_ih), ptr(c.weight_hh), ptr(c.bias_ih), ptr(c.bias_hh)]
            fold = getattr(self, '_fc2_fold', None)  # (tiger_hip.h: the GRU model's use of the upd_fc2 slot)
            if fold is not None:
                fc2 = TgLinear(ptr(fold), ptr(fold[3 * self.memory_dim * self.memory_dim:]))
        else:
            fc1, fc2 = lin(self.right_mem_updater.fn.fc1), lin(self.right_mem_updater.fn.fc2)
        L, R, S = self.left_memory, self.right_memory, self.msg_store
        mha = att.mha_fn
        m = TgModel(self.n_nodes, self.memory_dim, self.efeat_dim, self.n_neighbors, self.n_head,
                    0 if self.msg_src == 'left' else 1, 0 if self.upd_src == 'left' else 1,
                    _TSFM[self.msg_tsfm_type], _UPD[self.mem_update_type],
                    ptr(L.vals), ptr(L.update_ts), ptr(L.active_mask), ptr(R.vals), ptr(R.update_ts), ptr(R.active_mask),
                    ptr(S.node_msg_vals), ptr(S.node_msg_ts), ptr(S.has_msg_bits),
                    ptr(fg.nfeats), ptr(fg.efeats), ptr(self.time_encoder.basis_freq), ptr(self.time_encoder.phase),
                    tsfm1, tsfm2, gru[0], gru[1], gru[2], gru[3], fc1, fc2,
                    ptr(mha.q_proj_weight), ptr(mha.k_proj_weight), ptr(mha.v_proj_weight), ptr(mha.in_proj_bias),
                    lin(mha.out_proj), lin(att.merger.fc1), lin(att.merger.fc2),
                    ptr(self._fused) if self._fused is not None else None,
                    ptr(self._pending) if self._pending is not None else None,
                    ptr(self._row_of) if getattr(self, '_row_of', None) is not None else None,
                    ptr(self._gtab) if getattr(self, '_gtab', None) is not None else None,
                    ptr(self._ctab) if getattr(self, '_ctab', None) is not None else None)
        self._struct_cache = m
        return m

    # ---- eager updates (streaming with fixed parameters) ----------------------------------
    def eager_updates(self, enable: bool = True):
        """Streaming inference with FIXED parameters: h(t'+) of a node with a pending message is the same row
        every time the reference recomputes it (neither its mailbox row nor its memories change before the
        message is consumed), so `stream_step` / `launch_step` compute it ONCE, at the end of the batch that
        stores the message, into a [n_nodes, d] table; STEP 1-2 of later batches are then a gather of that
        table and the updater runs on the unique positive nodes of a batch instead of on every involved node
        with a pending message (C2: ~1 050 rows instead of ~4 200).  Same results as the lazy form.
        Every other method that touches state (restart, flush_msg, reset, contrast_learning, snapshots ...)
        is noticed and the table is rebuilt before the next eager step; after a parameter update or after
        writing to state tensors directly, call `invalidate_pending()`."""
        self._pending = None
        self._pending_stamp = None
        self._struct_cache = None
        if enable:
            self._pending = torch.zeros(self.msg_store.n, self.memory_dim, dtype=torch.float32, device=self.device)
        return self

    def partition_state(self, row_of: Tensor, n_rows: int):
        """PHYSICALLY partitioned state (multi-GPU; tiger_hip.h: tg_model.row_of): this process keeps `n_rows` rows of every
        state table - both memories, mailbox, has-message bitmap, eager-update table - instead of one per node.
        row_of[v] >= 0: the row of node v (rows the owner keeps for good); the caller re-points entries at arena rows for
        the nodes it pulls per batch.  Rows of nodes with row_of >= 0 are carried over from the current tables.  Node ids
        everywhere else (graph, batches, feature tables) stay global.  Only the partitioned engine's entry points address
        state by row: the model's own step / restart / flush methods must not be used on a partitioned model."""
        dev = self.device
        row_of = row_of.to(dev, torch.int32).contiguous()
        assert row_of.numel() == self.n_nodes and int(row_of.max()) < n_rows
        keep = torch.nonzero(row_of >= 0).flatten()
        rows = row_of[keep].long()
        prev = getattr(self, '_row_of', None)
        if prev is not None:  # already partitioned: the current tables are addressed by the CURRENT map
            src = prev.to(dev)[keep].long()
            if bool((src < 0).any()):
                raise ValueError('partition_state: a node gets a row that has none in the current partition')
            keep = src
        oldL, oldR, oldS, oldP = self.left_memory, self.right_memory, self.msg_store, self._pending
        L, R = Memory(n_rows, self.memory_dim).to(dev), Memory(n_rows, self.memory_dim).to(dev)
        S = MessageStoreNoGradLastOnly(n_rows, dim=self.raw_msg_dim).to(dev)
        for new, old in ((L, oldL), (R, oldR)):
            new.vals[rows] = old.vals[keep]
            new.update_ts[rows] = old.update_ts[keep]
            new.active_mask[rows] = old.active_mask[keep]
        S.node_msg_vals[rows] = oldS.node_msg_vals[keep]
        S.node_msg_ts[rows] = oldS.node_msg_ts[keep]
        has = rows[oldS._bits_of(keep).bool()]
        if has.numel():
            hip_ops.bitmap_mark(has, S.has_msg_bits, n_rows)
        self.left_memory, self.right_memory, self.msg_store = L, R, S
        self.msg_memory = L if self.msg_src == 'left' else R
        self.upd_memory = L if self.upd_src == 'left' else R
        self._row_of = row_of
        if oldP is not None:
            self._pending = torch.zeros(n_rows, self.memory_dim, dtype=torch.float32, device=dev)
            self._pending[rows] = oldP[keep]
        self._gtab = None
        self._ctab = None
        self._struct_cache = None
        self._pending_stamp = None
        self._touch()
        return self

    def invalidate_pending(self):
        self._pending_stamp = None
        self._gtab_stamp = None

    def _refuse_partitioned(self, what: str):
        """The model's own methods address state by NODE ID; on physically partitioned tables (partition_state: fewer rows
        than nodes) that would read and write other nodes' rows.  Only the partitioned engine's entry points (dist.py:
        embed-only lean step, serve / adopt / planned write-back / apply_messages on row lists) may run on such a model."""
        if getattr(self, '_row_of', None) is not None:
            raise RuntimeError(f'{what}: the model\'s state is physically partitioned (partition_state); only '
                               'www2023tiger_amd.dist.HipPartitionEngine may drive it')

    events = None              # the attached EventKeys tracker (track_events / attach_events), or None
    _events_admitting = False  # observe_events is inside its own call of observe / observe_late

    def _refuse_tracked(self, what: str):
        """With an event-key tracker attached (events.size == rows of the edge table, always) the calls that append or
        replace edge rows behind its back are refused: the rows they add would have no key and the invariant would
        break."""
        if self.events is not None and not self._events_admitting:
            raise RuntimeError(f'{what}: an event-key tracker is attached (model.events); feed the model through '
                               'observe_events, or detach_events() first (load a state, then attach_events the restored '
                               'tracker)')

    # ---- eager query rows (tiger_hip.h: tg_model.g_table) --------------------------------------------------------------
    def _gtab_wanted(self) -> bool:
        import os
        return (self._pending is not None and self._fused is not None and self.n_layers == 1
                and getattr(self, '_row_of', None) is None and os.environ.get('TG_GTAB', '1') != '0')

    def _sync_gtab(self):
        """The per-node table of folded attention queries G_v (one row per node; the fused eager step refreshes the rows of
        a batch's positive nodes itself): allocated when the model streams with eager updates AND pre-multiplied weights,
        rebuilt - all rows - whenever state or parameters changed outside that step."""
        if not self._gtab_wanted():
            if getattr(self, '_gtab', None) is not None:
                self._gtab = None
                self._ctab = None
                self._struct_cache = None
            return
        stamp = (self._state_stamp(), tuple(self._attn_stamp()), id(self._fused))
        if getattr(self, '_gtab', None) is not None and stamp == getattr(self, '_gtab_stamp', None):
            return
        if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('eager query rows: run one step eagerly before capturing it into a graph')
        dev, n = self.device, self.msg_store.n
        nk = self.n_head * (2 * self.memory_dim + (self.efeat_dim if self.raw_feat_getter.efeats is not None else 0))
        if getattr(self, '_gtab', None) is None or self._gtab.shape != (n, nk):
            self._gtab = torch.empty(n, nk, dtype=torch.float32, device=dev)
            # ... and the centre rows c_v = e(v) + nfeat(v) beside them (tg_model.c_table; TG_CTAB=0: without)
            self._ctab = (torch.empty(n, self.memory_dim, dtype=torch.float32, device=dev)
                          if os.environ.get('TG_CTAB', '1') != '0' else None)
            self._struct_cache = None
        m = self.model_struct()
        chunk = 262144
        ws = self._ws('gtab', min(n, chunk) * (4 * self.memory_dim + 4) + 64)
        for lo in range(0, n, chunk):
            ids = torch.arange(lo, min(n, lo + chunk), dtype=torch.int64, device=dev)
            check(lib.tg_attn_gtab_rows(C.byref(m), ids.numel(), ptr(ids), None, ptr(ws), ws.numel(), stream_ptr(dev)),
                  'tg_attn_gtab_rows')
        self._gtab_stamp = stamp

    def _tables_follow_restart(self, nids: Tensor):
        """restart(nids) has just run on a model whose per-node tables were current: the restarted nodes have no pending
        message any more and new memories (tiger.py:603-609), nothing else changed - their centre / query rows are recomputed
        (tg_attn_gtab_rows) and the tables are declared current again, instead of a rebuild over every node at the next
        eager step."""
        if self._pending is None:
            return
        if getattr(self, '_gtab', None) is not None:
            m = self.model_struct()
            n = int(nids.numel())
            ws = self._ws('gtab_r', n * (4 * self.memory_dim + 4) + 64)
            check(lib.tg_attn_gtab_rows(C.byref(m), n, ptr(nids), None, ptr(ws), ws.numel(), stream_ptr(self.device)),
                  'tg_attn_gtab_rows(restart)')
            self._gtab_stamp = (self._state_stamp(), tuple(self._attn_stamp()), id(self._fused))
        self._pending_stamp = self._state_stamp()

    def _touch(self):
        self._state_version += 1

    def _state_stamp(self):
        """What the eager-update table is a function of, as far as the host can see it: the explicit version counters of
        the model and its state modules, torch's own version counters of the state tensors (any in-place torch operation
        on a memory / mailbox tensor bumps them - the library's kernels, which write through raw pointers, do not) and
        those of the updater / message-transform parameters (an optimizer step is an in-place update).  Writes through
        .data / raw pointers by third parties remain invisible: invalidate_pending() is theirs to call."""
        L, R, S = self.left_memory, self.right_memory, self.msg_store
        tv = (L.vals._version, L.update_ts._version, R.vals._version, R.update_ts._version, S.node_msg_vals._version,
              S.node_msg_ts._version, S.has_msg_bits._version)
        pl = self._param_lists()[0]
        pv = sum([p._version for p in pl]) + (getattr(self, '_param_epoch', 0) << 32)
        return (self._state_version, id(L), L._version_, id(R), R._version_, id(S), S._version_, tv, pv)

    def _param_lists(self):
        """(updater + message-transform parameters, attention + time-encoder parameters) as plain lists - walking the
        module tree on every step costs more host time than the step's launches; reset when the tensors are re-homed"""
        pl = getattr(self, '_plists', None)
        if pl is None:
            upd = [p for mod in (self.right_mem_updater, self.msg_transform_fn) for p in mod.parameters()]
            att = [p for mod in (self.temporal_embedding_fn, self.time_encoder) for p in mod.parameters()]
            pl = self._plists = (upd, att)
        return pl

    def train(self, mode: bool = True):
        """Entering train() mode starts a new parameter epoch: everything derived from parameters (pre-multiplied attention
        weights, the eager-update and per-node tables) is rebuilt before its next use.  Their stamps are torch's version
        counters, which the library's optimizer (tg_adam_step - www2023tiger_amd.optim.Adam, FusedTrainer, also inside replayed
        graphs) does not bump: it writes through raw pointers.  Whoever trains passes through train() first."""
        if mode:
            self._param_epoch = getattr(self, '_param_epoch', 0) + 1
            self._mark_all('train(): parameters are about to change')
        return super().train(mode)

    def _attn_stamp(self):
        """versions of everything the pre-multiplied weights and the per-node tables built from them are made of: attention +
        time encoder, the updater's parameters (the table rows are updater outputs); + the parameter epoch (train())"""
        pl = self._param_lists()
        return [p._version for p in pl[1]] + [p._version for p in pl[0]] + [getattr(self, '_param_epoch', 0)]

    def _sync_pending(self):
        """Rebuild the table of precomputed updater rows if state changed outside the eager step:
        pending[v] = updater(upd_memory[v], tsfm(mailbox[v])) for every node with a pending message."""
        stamp = self._state_stamp()
        if stamp == self._pending_stamp:
            return
        if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('eager updates: run one step eagerly before capturing it into a graph')
        dev = self.device
        m = self.model_struct()
        n_rows = self.msg_store.n  # (= n_nodes unless the state is physically partitioned: the bitmap is over rows)
        comp = hip_ops.unique_compact(self.msg_store.has_msg_bits, n_rows, n_rows)
        n = int(comp['count'].item())
        if n:
            ids = comp['ids'][:n].contiguous()
            ids32 = ids.to(torch.int32)
            err = hip_ops.new_err(dev)
            nbytes = int(lib.tg_apply_messages_workspace_bytes(C.byref(m), n))
            ws = self._ws('apply', nbytes)
            check(lib.tg_apply_messages(C.byref(m), ptr(ids), ptr(ids32), ptr(comp['count']), n, ptr(self._pending),
                                        ptr(err), ptr(ws), ws.numel(), stream_ptr(dev)), 'tg_apply_messages(pending)')
            hip_ops.raise_if_err(err)
        self._pending_stamp = stamp

    def fuse_attention(self, enable: bool = True):
        """Inference with FIXED parameters: pre-multiply the attention weights (tg_attn_fuse) so that the
        embedding runs three products instead of six.  Call again after any parameter update; training
        ignores the fused weights."""
        self._fused = None
        self._fused_l1 = None
        self._fc2_fold = None
        self._struct_cache = None
        if not enable:
            return self
        blobs = []
        for layer in range(self.n_layers):  # every attention layer has its own weights (fns[layer])
            m = self.model_struct(layer)
            n = int(lib.tg_attn_fused_floats(C.byref(m)))
            if n == 0:
                raise RuntimeError('tg_attn_fuse: unsupported model dimensions')
            fused = torch.empty(n, dtype=torch.float32, device=self.device)
            nbytes = int(lib.tg_attn_fuse_workspace_bytes(C.byref(m)))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            check(lib.tg_attn_fuse(C.byref(m), ptr(fused), ptr(ws), nbytes, stream_ptr(self.device)), 'tg_attn_fuse')
            blobs.append(fused)
        self._fused = blobs[0]
        self._fused_l1 = blobs[1] if len(blobs) > 1 else None
        # the updater's memory-side weights folded through the merger's fc2 (tg_model.upd_fc2 of a GRU model): same life as the blob
        m = self.model_struct()
        n = int(lib.tg_gru_fc2_fold_floats(C.byref(m))) if self.n_layers == 1 else 0
        if n:
            fold = torch.empty(n, dtype=torch.float32, device=self.device)
            check(lib.tg_gru_fc2_fold(C.byref(m), ptr(fold), stream_ptr(self.device)), 'tg_gru_fc2_fold')
            self._fc2_fold = fold
        self._fused_stamp = self._attn_stamp()
        self._struct_cache = None
        return self

    def _ws(self, key, nbytes) -> Tensor:
        t = self._step_ws.get(key)
        if t is None or t.numel() < nbytes or t.device != self.device:
            t = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)
            self._step_ws[key] = t
        return t

    # ---- STEP 1-2 -----------------------------------------------------------------------
    def _consume(self, bitmap: Tensor, cap: int, err: Tensor):
        """involved / outdated decoding + reprs = right_memory[involved] with outdated rows
        replaced by updater(upd_memory, msg_fn(mailbox)) (tiger.py:208-221)."""
        m = self.model_struct()
        dev = self.device
        comp = hip_ops.unique_compact(bitmap, self.n_nodes, cap, and_bitmap=self.msg_store.has_msg_bits)  # bitmap is an input here
        reprs = torch.empty(cap, self.memory_dim, dtype=torch.float32, device=dev)
        s = stream_ptr(dev)
        check(lib.tg_mailbox_consume_gather(C.byref(m), ptr(comp['ids']), ptr(comp['count']), cap, ptr(reprs), s),
              'tg_mailbox_consume_gather')
        nbytes = int(lib.tg_apply_messages_workspace_bytes(C.byref(m), cap))
        ws = self._ws('apply', nbytes)
        check(lib.tg_apply_messages(C.byref(m), ptr(comp['and_ids']), ptr(comp['and_pos']), ptr(comp['and_count']),
                                    cap, ptr(reprs), ptr(err), ptr(ws), ws.numel(), s), 'tg_apply_messages')
        return comp, reprs

    def compute_messages(self, node_ids: Union[Tensor, np.ndarray, None] = None):
        """tiger.py:292-337 standalone form: (outdated ids, transformed messages, message ts)."""
        self._refuse_partitioned('compute_messages')
        outdated = self.msg_store.get_outdated_node_ids(node_ids).to(self.device)
        if len(outdated) == 0:
            return outdated, None, None
        last = self.msg_memory.update_ts[outdated]
        raw, ts = self.msg_aggregate_fn(outdated, last, self.msg_store.node_messages)
        if self.msg_src == 'left' and not (ts == last).all().item():
            raise ValueError("Messages' ts should be equal to last update ts when using left memory as msg source.")
        return outdated, self.msg_transform_fn(raw.detach()), ts

    # ---- the batch ----------------------------------------------------------------------
    def _train_forward(self, src_ids, dst_ids, neg_dst_ids, ts, eids, computation_graph, mutual: bool):
        """Training mode with autograd enabled: the whole iteration (collate, STEP 1-7, backward,
        write-back) runs as one tg_train_step; the returned losses carry an autograd node that
        hands the finished gradients to the parameters when `.backward()` is called."""
        from .training import TrainBuffers, hand_over
        self._touch()
        dev = self.device
        B = len(src_ids)
        key = ('train', B, mutual)
        tb = self._step_ws.get(key)
        if tb is None:
            tb = TrainBuffers(self, B, mutual=mutual)
            self._step_ws[key] = tb
        ts64 = getattr(computation_graph, 'ts64', None)  # the collator keeps the float64 event times
        if ts64 is None:
            ts64 = ts.to(dev).double()
        to = lambda x: x.to(dev).long()
        tb.sb.load(to(src_ids), to(dst_ids), to(neg_dst_ids), ts64, to(eids))
        cg_graph = getattr(computation_graph, 'graph', None)
        if cg_graph is None and hasattr(computation_graph, 'ts64'):
            raise NotImplementedError("training on device samples with strategy='recent_edges'")
        # every parameter owned by www2023tiger_amd.optim.Adam: nothing is read back in this iteration (the
        # invariant word of this batch is checked at the next one / flush_msg(), the live flags stay on the device)
        deferred = tb.err_host is not None and all(getattr(p, '_tg_deferred', False) for _, p, _ in tb.params)
        self._poll_train_errors()
        tb.launch(graph=cg_graph)  # sample where the collator sampled
        if deferred:
            tb.err_host[:1].copy_(tb.sb.err, non_blocking=True)
            tb.err_host[1:].copy_(tb.sb.counts[1:2], non_blocking=True)
            tb.err_event = torch.cuda.Event()
            tb.err_event.record()
        else:
            word = int(tb.sb.err.item())
            self.note_rows(int(tb.sb.counts[1].item()))
            if word:
                tb.sb.err.zero_()
                from .._lib import raise_invariants
                raise_invariants(word & 0xFFFFFFFF)
        grads = [(tb.grads[name], 1 if group == 2 else 0, group) for name, _, group in tb.params]
        losses = hand_over(tb.losses, grads, tb.flags if deferred else tb.flags.clone(),
                           [p for _, p, _ in tb.params], tb if deferred else None)
        return (losses, tb.sb.h[:2 * B].clone(), tb.pos_scores.clone(), tb.neg_scores.clone(),
                tb.sb.h_prev_left.clone(), tb.sb.h_prev_right.clone())

    def _poll_train_errors(self):
        """Deferred invariant check of the train steps launched without a read-back."""
        for key, tb in self._step_ws.items():
            ev = getattr(tb, 'err_event', None)
            if ev is None:
                continue
            ev.synchronize()
            tb.err_event = None
            word = int(tb.err_host[0].item())
            self.note_rows(int(tb.err_host[1].item()))
            if word:
                tb.sb.err.zero_()
                from .._lib import raise_invariants
                raise_invariants(word & 0xFFFFFFFF)

    def contrast_learning(self, src_ids: Tensor, dst_ids: Tensor, neg_dst_ids: Tensor, ts: Tensor, eids: Tensor,
                          computation_graph) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
        """tiger.py:174-290 -> (contrast_loss, h_left, pos_scores, neg_scores, h_prev_left, h_prev_right)"""
        self._refuse_partitioned('contrast_learning')
        if self.training and torch.is_grad_enabled():
            losses, *rest = self._train_forward(src_ids, dst_ids, neg_dst_ids, ts, eids, computation_graph, False)
            return (losses[0], *rest)
        with torch.no_grad():
            if (getattr(computation_graph, 'ts64', None) is not None
                    and getattr(computation_graph, 'graph', None) is not None and self._fused_eval_ok(computation_graph.graph)):
                return self._contrast_learning_fused_eval(src_ids, dst_ids, neg_dst_ids, eids, computation_graph)
            return self._contrast_learning_eval(src_ids, dst_ids, neg_dst_ids, ts, eids, computation_graph)

    def _fused_eval_ok(self, graph=None) -> bool:
        """does the one-call evaluation step (tg_train_step without gradient buffers) apply?  One or two layers, the
        recent-edges / recent-nodes / uniform strategies"""
        if self.hit_type == 'vec' and (2 * (self.nfeat_dim + self.n_neighbors)) % 4:
            return False  # the score head's pair rows must be float4-aligned
        strategy = getattr(graph if graph is not None else self.graph, 'strategy', 'recent_edges')
        return self.n_layers in (1, 2) and strategy in ('recent_edges', 'recent_nodes', 'uniform')

    def _contrast_learning_fused_eval(self, src_ids, dst_ids, neg_dst_ids, eids, computation_graph):
        """no_grad / eval(): collate, STEP 1-7 and the write-back as ONE device call (tg_train_step without
        gradient buffers).  The computation graph only contributes the float64 event times: the step
        samples the same neighbourhoods itself."""
        from .training import TrainBuffers
        dev = self.device
        B = len(src_ids)
        key = ('eval', B)
        tb = self._step_ws.get(key)
        if tb is None:
            tb = TrainBuffers(self, B, eval_only=True)
            self._step_ws[key] = tb
        to = lambda x: x.to(dev).long()
        tb.sb.load(to(src_ids), to(dst_ids), to(neg_dst_ids), computation_graph.ts64, to(eids))
        # the collator's graph, not model.graph: the reference embeds with the neighbourhoods the collator
        # sampled (e.g. warm-up batches are collated on the training graph while model.graph is the full one)
        self._poll_train_errors()  # invariant word of the previous batch (read back asynchronously, no stall)
        tb.launch(graph=getattr(computation_graph, 'graph', None))
        if tb.err_host is not None:
            tb.err_host[:1].copy_(tb.sb.err, non_blocking=True)
            tb.err_host[1:].copy_(tb.sb.counts[1:2], non_blocking=True)
            tb.err_event = torch.cuda.Event()
            tb.err_event.record()
        else:
            word = int(tb.sb.err.item())
            if word:
                tb.sb.err.zero_()
                from .._lib import raise_invariants
                raise_invariants(word & 0xFFFFFFFF)
        return (tb.losses[0].clone(), tb.sb.h[:2 * B].clone(), tb.pos_scores.clone(), tb.neg_scores.clone(),
                tb.sb.h_prev_left.clone(), tb.sb.h_prev_right.clone())

    def _contrast_learning_eval(self, src_ids, dst_ids, neg_dst_ids, ts, eids, computation_graph):
        cg = computation_graph
        self._touch()
        dev = self.device
        m = self.model_struct()
        s = stream_ptr(dev)
        bs, d = len(src_ids), self.memory_dim
        src_ids, dst_ids, neg_dst_ids, eids = (x.to(dev).long().contiguous() for x in
                                               (src_ids, dst_ids, neg_dst_ids, eids))
        self._mark(src_ids)  # STEP 4-6 below write the rows of the positive nodes
        self._mark(dst_ids)
        ts = ts.to(dev).float().contiguous()
        pos = torch.cat([src_ids, dst_ids])
        batch_ids = torch.cat([pos, neg_dst_ids])
        ts2, ts3 = ts.repeat(2), ts.repeat(3)
        err = hip_ops.new_err(dev)
        K = self.n_neighbors
        cap = 3 * bs * (1 + K + (K * K if self.n_layers == 2 else 0))
        comp, reprs = self._consume(cg.bitmap, cap, err)  # STEP 1-2
        h_all = self.temporal_embedding_fn.compute_embedding_with_computation_graph(  # STEP 3
            reprs, batch_ids, ts3, cg, m if self.n_layers == 1 else self.model_struct, comp['rank'])
        upos, index = hip_ops.select_latest_nids(pos, ts2, self.n_nodes)  # dedup (tiger.py:232,419; memory.py:98)
        n_upos = torch.tensor([len(upos)], dtype=torch.int32, device=dev)
        check(lib.tg_consume_update_right(C.byref(m), ptr(upos), ptr(n_upos), len(upos), ptr(reprs), ptr(cg.bitmap),
                                          ptr(comp['rank']), ptr(err), s), 'tg_consume_update_right')  # STEP 4
        check(lib.tg_store_events(C.byref(m), bs, ptr(src_ids), ptr(dst_ids), ptr(ts), ptr(eids), ptr(upos),
                                  ptr(index), ptr(n_upos), ptr(err), s), 'tg_store_events')  # STEP 5
        h_prev_left = hip_ops.gather_rows(self.left_memory.vals, pos)  # restarter targets (tiger.py:248-251)
        h_prev_right = hip_ops.gather_rows(self.right_memory.vals, pos)
        h_left = h_all[:2 * bs]
        hip_ops.memory_scatter(self.left_memory.vals, self.left_memory.update_ts, self.left_memory.active_mask,
                               upos, h_all, ts2, src_index=index, check_past=True, err=err)  # STEP 6
        hip_ops.raise_if_err(err)
        # STEP 7 (tiger.py:257-288): score head, plain torch (outside the accelerated path)
        x, y, neg_y = h_all.reshape(3, bs, d)
        pos_scores, neg_scores = self._scores(x, y, neg_y, cg.hit_data)
        labels = torch.cat([torch.ones_like(pos_scores), torch.zeros_like(neg_scores)])
        loss = self.contrast_loss_fn(torch.cat([pos_scores, neg_scores]), labels)
        return loss, h_left, pos_scores, neg_scores, h_prev_left, h_prev_right

    def _scores(self, x, y, neg_y, hit_data):
        if self.hit_type in ('vec', 'bin', 'count'):
            sh, dh, nsh, ndh = hit_data
        if self.hit_type == 'vec':
            xp, yp = torch.cat([x, sh], 1), torch.cat([y, dh], 1)
            xn, yn = torch.cat([x, nsh], 1), torch.cat([neg_y, ndh], 1)
        elif self.hit_type in ('bin', 'count'):
            red = (lambda t: t.max(1).values.long()) if self.hit_type == 'bin' else (lambda t: t.sum(1).long())
            e = self.hit_embedding
            xp, yp, xn, yn = x + e(red(sh)), y + e(red(dh)), x + e(red(nsh)), neg_y + e(red(ndh))
        else:
            xp = xn = x
            yp, yn = y, neg_y
        return self.score_fn(xp, yp).squeeze(1), self.score_fn(xn, yn).squeeze(1)

    # ---- ranking evaluation (one-vs-many) -------------------------------------------------
    # rows of every embedding call of rank_scores.  The library chooses the kernels of the attention products and of the
    # updater by the row count (K-split variants for launches that do not fill the chip), so the bits of an embedding
    # depend on how many rows it was computed among; a fixed count makes a score a function of its pair and the state alone
    RANK_EMBED_ROWS = 4096

    def rank_scores(self, src_ids: Tensor, dst_ids: Tensor, ts: Tensor, cand: Tensor, *, chunk_queries: int = 65536,
                    graph=None, uptodate: Optional[Tensor] = None) -> Tensor:
        """scores [B, 1 + C] of every event's true destination (column 0) and of its C candidate destinations cand[i, :]
        on the model's CURRENT state: column 0 is `pos_scores` of contrast_learning on this batch, column 1 + j its
        `neg_scores` had the negatives been cand[:, j] (tiger.py:174-288) - STEP 1-3 over the flat list of B (2 + C)
        (node, t) queries on the operator path, the score head over all pairs as one call (tg_rank_scores); STEP 4-6 never
        run and NOTHING is written: memories, mailbox and derived tables are what they were.  ts: the event times, float64
        where the caller has them (the sampler searches float64).  cand: int64 [B, C], or [C] shared by all events.
        Events are processed in chunks of at most `chunk_queries` queries (at least one event), so the workspace is bounded
        whatever C is; a score does not depend on the chunking, nor on B or C: every query is embedded in a call of
        exactly RANK_EMBED_ROWS rows (see there).  graph: the graph neighbourhoods are sampled from
        (default: model.graph; an evaluation loop passes its collator's).  eval() mode only.  Refused before anything
        runs: strategy 'uniform' (a score would depend on the graph's random stream), a partitioned model, 'vec' hits with
        2 (d + K) not a multiple of 4 (as the one-call evaluation step).
        uptodate (a bitmap of hip_ops.new_bitmap; TIGER only): lazy restarts - this form WRITES MEMORIES.  Before anything
        is embedded, ONE `restart_involved` over all B (2 + C) queries restarts every node their embeddings will read
        that the bitmap does not hold yet, at the earliest event time, and marks it in the bitmap; the scores are then
        those of the plain form on that state.  The restart never runs per chunk, so a score still does not depend on
        `chunk_queries`.  A model without a restarter raises NotImplementedError."""
        graph, strategy = self._pair_refusals('rank_scores', graph, chunk_queries, uptodate)
        dev = self.device
        src_ids, dst_ids = (x.to(dev).long().contiguous() for x in (src_ids, dst_ids))
        cand = torch.as_tensor(cand).to(dev).long()
        B = src_ids.numel()
        if cand.dim() == 1:
            cand = cand.unsqueeze(0).expand(B, -1)
        if cand.dim() != 2 or cand.shape[0] != B or dst_ids.numel() != B or ts.numel() != B:
            raise ValueError(f'rank_scores: {B} events, dst {tuple(dst_ids.shape)}, ts {tuple(ts.shape)}, cand {tuple(cand.shape)}')
        ids_all = torch.cat([dst_ids[:, None], cand], 1)
        if uptodate is not None:
            self._restart_pairs(src_ids, ids_all, ts, uptodate, graph)
        return self._pair_scores('rank_scores', src_ids, ids_all, ts, graph, strategy, chunk_queries)

    def _pair_refusals(self, what: str, graph, chunk_queries: int, uptodate=None):
        """what rank_scores and recommend refuse before anything runs -> (graph, its sampling strategy)"""
        self._refuse_partitioned(what)
        if uptodate is not None and getattr(self, 'restarter_fn', None) is None:
            raise NotImplementedError(f'{what}: lazy restarts (uptodate) need a model with a restarter (TIGER)')
        graph = self.graph if graph is None else graph
        strategy = getattr(graph, 'strategy', 'recent_edges')
        if strategy not in ('recent_edges', 'recent_nodes'):
            raise NotImplementedError(f"{what} samples 'recent_edges' or 'recent_nodes'; strategy={strategy!r} would make a "
                                      "score depend on the graph's random stream")
        if self.n_layers not in (1, 2):
            raise NotImplementedError(f'{what}: the operator path embeds with n_layers 1 or 2')
        if self.hit_type == 'vec' and (2 * (self.memory_dim + self.n_neighbors)) % 4:
            raise NotImplementedError(f"{what}: 'vec' hits need 2 (d + n_neighbors) to be a multiple of 4")
        if self.training:
            raise RuntimeError(f'{what} scores the model in eval() mode')
        if chunk_queries < 1:
            raise ValueError('chunk_queries must be positive')
        self.check_graph(graph)
        if uptodate is not None:
            self._check_uptodate(what, uptodate)
        return graph, strategy

    def _check_uptodate(self, what: str, uptodate):
        if torch.is_tensor(uptodate) and uptodate.numel() != hip_ops.bitmap_words(self.n_nodes):
            raise ValueError(f'{what}: the uptodate bitmap holds {uptodate.numel()} words, {self.n_nodes} node ids take '
                             f'{hip_ops.bitmap_words(self.n_nodes)} - after grow_nodes / observe(num_node=) pass '
                             'hip_ops.bitmap_grown(uptodate, model.n_nodes)')

    def _restart_pairs(self, src_ids: Tensor, ids_all: Tensor, ts: Tensor, uptodate: Tensor, graph) -> int:
        """the lazy restart of rank_scores / recommend: ONE `restart_involved` over the flat query list `_pair_scores`
        embeds chunk by chunk - the sources, then ids_all [B, C1] flattened, each at its event's time"""
        dev = self.device
        ts64 = ts.to(dev).double().contiguous().reshape(-1)
        nodes = torch.cat([src_ids, ids_all.reshape(-1)])
        return self.restart_involved(nodes, torch.cat([ts64, ts64.repeat_interleave(ids_all.shape[1])]), uptodate, graph=graph)

    def _embed_prepare(self):
        """before a read-only embedding pass: pending invariant words are polled and pre-multiplied attention weights
        follow the parameters, as before a streaming / evaluation step; the eager update and query-row tables are neither
        read (the operator path consumes the mailbox itself) nor made stale (no state changes): they stay as they are"""
        self._poll_train_errors()
        if self._fused is not None and self._fused_stamp != self._attn_stamp():
            self.fuse_attention()

    def _embed_queries(self, nodes: Tensor, t64: Tensor, graph, strategy: str, err: Tensor):
        """STEP 1-3 of the flat (node, time) queries on the current state, nothing written -> (h float32 [Q, d], nb int64
        [Q, K] recent-edges neighbour ids, None for hit_type 'none').  The embedding unit of rank_scores, recommend and
        embed_catalogue: exactly RANK_EMBED_ROWS queries per call (the last unit filled up with copies of its last query)
        and one involved-set capacity - the products and the updater pick their kernel, K-split or not, by the row count,
        and a K split sums in another order, so a query embedded among another number of rows could round differently.
        Every query meets the same kernels whatever the list holds: its bits are a function of (node, time, state).
        no_grad, after `_embed_prepare`; nodes int64 [Q] and t64 float64 [Q] on the model's device."""
        from ..data.data_loader import GraphCollator
        d, K, dev = self.memory_dim, self.n_neighbors, self.device
        coll = GraphCollator(graph, K, self.n_layers)
        hits = self.hit_type != 'none'
        R = self.RANK_EMBED_ROWS
        cap = min(R * (1 + K + (K * K if self.n_layers == 2 else 0)), self.n_nodes)
        Q = nodes.numel()
        h = torch.empty(Q, d, dtype=torch.float32, device=dev)
        nb = torch.empty(Q, K, dtype=torch.int64, device=dev) if hits else None
        for off in range(0, Q, R):
            n = min(R, Q - off)
            qn, qt = nodes[off:off + n], t64[off:off + n]
            if n < R:
                qn = torch.cat([qn, qn[-1:].expand(R - n)])
                qt = torch.cat([qt, qt[-1:].expand(R - n)])
            layers, bitmap, _ = coll.collate_memory_nodes(qn.contiguous(), qt.contiguous())
            comp, reprs = self._consume(bitmap, cap, err)  # STEP 1-2, read-only
            cg = _QueryGraph(layers, bitmap)
            m = self.model_struct()
            hq = self.temporal_embedding_fn.compute_embedding_with_computation_graph(  # STEP 3
                reprs, qn, qt.float(), cg, m if self.n_layers == 1 else self.model_struct, comp['rank'])
            h[off:off + n] = hq[:n]
            if hits:  # hit windows are recent-edges lists whatever the graph's strategy (data_loader.py:61-75)
                nbq = layers[-1][0] if strategy == 'recent_edges' else graph.sample_device(
                    qn, qt, K, strategy='recent_edges', want_dirs=False)[0]
                nb[off:off + n] = nbq[:n]
        return h, nb

    def _check_ids(self, ids: Tensor, message: str):
        """ValueError(message) if a node id of the non-empty int64 tensor `ids` lies outside [0, n_nodes)"""
        lo_id, hi_id = torch.aminmax(ids)
        if int(lo_id) < 0 or int(hi_id) >= self.n_nodes:
            raise ValueError(message)

    def _pair_scores(self, what: str, src_ids: Tensor, ids_all: Tensor, ts: Tensor, graph, strategy: str,
                     chunk_queries: int) -> Tensor:
        """scores [B, C1] of the pairs (src_ids[i], ids_all[i, j]) at ts[i] on the current state, nothing written (the body
        of rank_scores, which passes [dst | cand]; recommend passes its candidates alone).  C1 >= 1; `_pair_refusals` has
        run; src_ids int64 [B] and ids_all int64 [B, C1] live on the model's device."""
        from .training import score_struct
        d, K, dev = self.memory_dim, self.n_neighbors, self.device
        B = src_ids.numel()
        if B:
            self._check_ids(torch.cat([src_ids, ids_all.reshape(-1)]), f'{what}: a node id outside [0, n_nodes)')
        ts64 = ts.to(dev).double().contiguous()
        C1 = ids_all.shape[1]
        scores = torch.empty(B, C1, dtype=torch.float32, device=dev)
        if B == 0:
            return scores
        with torch.no_grad():
            self._embed_prepare()
            sp = score_struct(self)
            hits = self.hit_type != 'none'
            err = hip_ops.new_err(dev)
            s = stream_ptr(dev)
            step = max(1, int(chunk_queries) // (C1 + 1))
            for lo in range(0, B, step):
                hi = min(B, lo + step)
                b = hi - lo
                ids = ids_all[lo:hi].contiguous()
                nodes = torch.cat([src_ids[lo:hi], ids.reshape(-1)])
                t64 = torch.cat([ts64[lo:hi], ts64[lo:hi].repeat_interleave(C1)])
                h, nb = self._embed_queries(nodes, t64, graph, strategy, err)
                nb_src = nb_cand = None
                if hits:
                    nb_src, nb_cand = nb[:b], nb[b:]
                nbytes = int(lib.tg_rank_scores_workspace_bytes(b, d, C.byref(sp)))
                ws = self._ws('rank', nbytes)
                out = scores[lo:hi]
                check(lib.tg_rank_scores(b, C1 - 1, d, K, C.byref(sp), ptr(h[:b]), ptr(h[b:]), ptr(nb_src), ptr(nb_cand),
                                         ptr(nodes[:b]), ptr(ids), ptr(out), ptr(ws), ws.numel(), s), 'tg_rank_scores')
            hip_ops.raise_if_err(err)
        return scores

    # ---- top-k recommendation ------------------------------------------------------------
    def _snapshot_stamp(self):
        """what a catalogue snapshot's rows are a function of, as far as the host can see it: the state (as for the eager-
        update table), the number of steps run on this model, the attention / updater parameters"""
        return (self._state_stamp(), getattr(self, '_step_serial', 0), tuple(self._attn_stamp()))

    def _score_stamp(self):
        w = self.score_fn.fc1.weight
        return (w._version, w.data_ptr(), getattr(self, '_param_epoch', 0))

    def _make_snapshot(self, cand: Tensor, t: float, graph, strategy: str) -> CatalogueSnapshot:
        dev = self.device
        with torch.no_grad():
            self._embed_prepare()
            err = hip_ops.new_err(dev)
            t64 = torch.full((cand.numel(),), t, dtype=torch.float64, device=dev)
            h, nb = self._embed_queries(cand, t64, graph, strategy, err)
            hip_ops.raise_if_err(err)
        snap = CatalogueSnapshot(self, cand, h, nb, t, graph, self._snapshot_stamp())
        if self._tracker is not None:  # (nothing is cleared: bits from before the snapshot only over-mark)
            snap.change_epoch = self._tracker.epoch
        return snap

    def refresh_catalogue(self, snap: CatalogueSnapshot, t: float, *, max_age: Optional[float] = None, graph=None,
                          clear: bool = True, verify: bool = False) -> CatalogueSnapshot:
        """Refresh a catalogue snapshot incrementally: re-embed, at time t, only the rows that read something that changed
        since they were computed -> a NEW CatalogueSnapshot over the same ids; `snap` stays valid and unchanged.  Needs
        `track_changes()` switched on before `snap` was made.  The child carries t_row float64 [C] and obeys ONE
        invariant: for every row j, h[j], nb[j] and (when present) P[j] are, bit for bit, what embed_catalogue(ids[j:j+1],
        t_row[j]) followed by tg_rank_cand_half gives on the model's CURRENT state, graph and parameters.  Row j is dirty
        iff (1) a node of involved(ids[j], t_row[j]) - the set of tg_involved_list on the current graph - has its bit in
        the tracker, or (2) max_age is given and t - t_row[j] > max_age (strict float64), or (3) the tracker's `whole`
        flag is set or the attention / updater parameters changed since `snap` (then every row).  Dirty rows are embedded
        at t (`_embed_queries`: a row's bits are a function of (node, time, state)) and get t_row[j] = t; clean rows keep
        their bits and their time.  The child's t is t, its stamps are the current ones (recommend accepts it without
        stale_ok) and `last_refreshed` = (n_dirty, rows dirty by age alone); when every row is dirty by rule (3) the
        dirty pass is skipped and the second number is 0 whatever the rows' ages and `max_age`.  One value is read back:
        the count.
        Nothing is written to the model's state.  clear=True clears the tracker afterwards and gives the child the new
        epoch (the parent can then not be refreshed again); clear=False keeps bits and epoch, for a caller with several
        snapshots.  verify=True re-embeds, for every distinct time of the child, the rows of that time and raises
        RuntimeError naming the first row whose bits differ - a debugging aid for a missed change, not the fast path.
        Refused before anything runs, with snapshot and tracker unchanged: no tracker; a snapshot from another tracker
        epoch; a snapshot of another model, device or numbering; t NaN or below snap.t; max_age negative or NaN; whatever
        embed_catalogue refuses (strategy 'uniform', a partitioned model, training mode, the 'vec' cases)."""
        from .training import score_struct
        tr = self._tracker
        if tr is None:
            raise RuntimeError('refresh_catalogue: nothing recorded what changed - call track_changes() before embed_catalogue')
        if not isinstance(snap, CatalogueSnapshot):
            raise TypeError(f'refresh_catalogue: {type(snap).__name__} is no CatalogueSnapshot')
        graph, strategy = self._pair_refusals('refresh_catalogue', graph, 1, None)
        self._shared_refusals('refresh_catalogue')
        if self.memory_dim % 4 or self.n_neighbors > TG_INVOLVED_MAX_K:
            raise NotImplementedError(f'refresh_catalogue: memory_dim {self.memory_dim} must be a multiple of 4 (the merge moves '
                                      f'16-byte words) and n_neighbors {self.n_neighbors} at most {TG_INVOLVED_MAX_K}')
        self._check_snapshot(snap, graph, True)
        if snap.change_epoch != tr.epoch:
            raise RuntimeError(f'refresh_catalogue: the snapshot belongs to change epoch {snap.change_epoch}, the tracker is at '
                               f'{tr.epoch} (cleared by another refresh, or the snapshot predates track_changes): embed it again')
        t = float(t)
        if t != t or t < snap.t:
            raise ValueError(f'refresh_catalogue: t = {t}; a refresh moves a snapshot of time {snap.t} forward')
        if max_age is not None and not float(max_age) >= 0.0:
            raise ValueError(f'refresh_catalogue: max_age = {max_age} (a non-negative number of time units)')
        dev, Cn = self.device, len(snap)
        K = self.n_neighbors
        t_old = snap.t if snap.t_row is None else snap.t_row
        whole = tr.whole or tuple(snap.stamp[2]) != tuple(self._attn_stamp())
        with torch.no_grad():
            self._embed_prepare()
            if whole or Cn == 0:
                n_dirty, n_age = Cn, 0
                rank = torch.arange(Cn, dtype=torch.int32, device=dev)
                ids_new = snap.ids
            else:
                out = hip_ops.catalogue_dirty(graph, snap.ids, t_old, K, self.n_layers, tr.bits, t, max_age=max_age,
                                              strategy=strategy, check_ids=False)  # (embed_catalogue checked them)
                n_dirty, n_age = (int(x) for x in out['count'].tolist())  # the one read-back
                rank = out['rank']
                ids_new = snap.ids[out['cols'][:n_dirty].long()]
            err = hip_ops.new_err(dev)
            h_new = torch.empty(0, self.memory_dim, dtype=torch.float32, device=dev)
            nb_new = None if snap.nb is None else torch.empty(0, K, dtype=torch.int64, device=dev)
            if n_dirty:
                t64 = torch.full((n_dirty,), t, dtype=torch.float64, device=dev)
                h_new, nb_new = self._embed_queries(ids_new.contiguous(), t64, graph, strategy, err)
                hip_ops.raise_if_err(err)
            P_old = P_new = None
            score_stamp = self._score_stamp()
            if snap._P is not None and snap._P_stamp == score_stamp:
                P_old, P_new = snap._P, torch.empty_like(h_new)
                if n_dirty:
                    sp = score_struct(self)
                    check(lib.tg_rank_cand_half(n_dirty, self.memory_dim, K, C.byref(sp), ptr(h_new), ptr(P_new),
                                                stream_ptr(dev)), 'tg_rank_cand_half')
            if Cn:
                h, P, nb, t_row = hip_ops.catalogue_merge(rank, n_dirty, snap.h, h_new, t_old, t, P_old=P_old, P_new=P_new,
                                                          nb_old=snap.nb, nb_new=nb_new)
            else:
                h, P, nb, t_row = snap.h.clone(), None, snap.nb, torch.empty(0, dtype=torch.float64, device=dev)
        child = CatalogueSnapshot(self, snap.ids, h, nb, t, graph, self._snapshot_stamp())
        child.t_row = t_row
        child.change_epoch = tr.epoch
        if P is not None:
            child._P, child._P_stamp = P, score_stamp
        if snap._col_of is not None and child.n_nodes == snap.n_nodes:
            child._col_of = snap._col_of
        if verify:
            self._verify_snapshot(child, graph, strategy)
        self.last_refreshed = (n_dirty, n_age)
        if clear:
            tr.clear()
            child.change_epoch = tr.epoch
        return child

    def _verify_snapshot(self, snap: CatalogueSnapshot, graph, strategy: str):
        """refresh_catalogue(verify=True): every group of rows that share a t_row, embedded again at that time"""
        from .training import score_struct
        dev = self.device
        with torch.no_grad():
            for tau in torch.unique(snap.t_row).tolist():
                rows = torch.nonzero(snap.t_row == tau).reshape(-1)
                err = hip_ops.new_err(dev)
                t64 = torch.full((rows.numel(),), tau, dtype=torch.float64, device=dev)
                h, nb = self._embed_queries(snap.ids[rows].contiguous(), t64, graph, strategy, err)
                hip_ops.raise_if_err(err)
                pairs = [('h', h, snap.h[rows])]
                if nb is not None:
                    pairs.append(('nb', nb, snap.nb[rows]))
                if snap._P is not None:
                    P = torch.empty_like(h)
                    sp = score_struct(self)
                    check(lib.tg_rank_cand_half(rows.numel(), self.memory_dim, self.n_neighbors, C.byref(sp), ptr(h), ptr(P),
                                                stream_ptr(dev)), 'tg_rank_cand_half')
                    pairs.append(('P', P, snap._P[rows]))
                for name, fresh, held in pairs:
                    a = fresh.view(torch.int32) if fresh.dtype == torch.float32 else fresh
                    b = held.contiguous().view(torch.int32) if held.dtype == torch.float32 else held
                    bad = (a != b).reshape(rows.numel(), -1).any(1)
                    if bool(bad.any()):
                        j = int(rows[torch.nonzero(bad)[0, 0]])
                        raise RuntimeError(f'refresh_catalogue(verify=True): row {j} (node {int(snap.ids[j])}, embedded at '
                                           f'{tau}) differs from a fresh embedding in {name} - a change the tracker did '
                                           'not see (a write through a raw tensor? `tracker.mark(ids)` is the caller\'s)')

    def embed_catalogue(self, cand: Tensor, t: float, *, graph=None, uptodate: Optional[Tensor] = None) -> CatalogueSnapshot:
        """Embed a shared catalogue once, at ONE time t, on the model's CURRENT state -> CatalogueSnapshot (ids, h, nb, t;
        see there).  cand: int64 [C]; duplicates and the padding id 0 are allowed as in recommend.  t: one float64 time.
        The C queries (cand[j], t) run through the embedding unit of rank_scores / recommend (`_embed_queries`), so an
        item's row holds the bits recommend's per-pair path computes for the query (cand[j], t).  NOTHING is written,
        unless `uptodate` (a bitmap of hip_ops.new_bitmap; TIGER only) is given: then ONE `restart_involved` over the C
        queries runs first, as in recommend's lazy form, and `last_restarted` holds its count.  Refused before anything
        runs: whatever recommend refuses (strategy 'uniform', a partitioned model, training mode, unaligned 'vec' hits),
        'vec' hits with an odd memory_dim (tg_rank_scores_shared), a NaN time, an id outside [0, n_nodes)."""
        graph, strategy = self._pair_refusals('embed_catalogue', graph, 1, uptodate)
        self._shared_refusals('embed_catalogue')
        cand = torch.as_tensor(cand).to(self.device).long().contiguous()
        if cand.dim() != 1:
            raise ValueError(f'embed_catalogue: cand {tuple(cand.shape)}; a catalogue is int64 [C]')
        t = float(t)
        if t != t:
            raise ValueError('embed_catalogue: t is NaN')
        if cand.numel():
            self._check_ids(cand, 'embed_catalogue: a node id outside [0, n_nodes)')
        if uptodate is not None and cand.numel():
            self.restart_involved(cand, torch.full((cand.numel(),), t, dtype=torch.float64, device=self.device), uptodate,
                                  graph=graph)
        return self._make_snapshot(cand, t, graph, strategy)

    def _shared_refusals(self, what: str):
        if self.hit_type == 'vec' and self.memory_dim % 2:
            raise NotImplementedError(f"{what}: 'vec' hits on a catalogue snapshot need an even memory_dim")

    def _check_snapshot(self, snap: CatalogueSnapshot, graph, stale_ok: bool):
        if snap.model is not self:
            raise ValueError('recommend: the catalogue snapshot was embedded by another model')
        if snap.device != self.device:
            raise ValueError(f'recommend: the catalogue snapshot lives on {snap.device}, the model on {self.device}')
        # (a snapshot from before the model admitted node ids - grow_nodes - is stale like one from before any observe)
        # (growth bumps the state stamp; a snapshot over fewer ids whose stamp is current did not come from this model's past)
        stale = snap.stamp != self._snapshot_stamp() or snap.graph_serial != getattr(graph, 'serial', None)
        if snap.n_nodes > self.n_nodes or (snap.n_nodes < self.n_nodes and not stale) or snap.h.shape[1] != self.memory_dim:
            raise ValueError(f'recommend: the catalogue snapshot covers {snap.n_nodes} node ids, the model {self.n_nodes}')
        if not stale_ok and stale:
            raise RuntimeError('recommend: the catalogue snapshot is stale - the state, the parameters or the graph have '
                               'changed since embed_catalogue (stream_step / observe / forget / a restart).  Embed it '
                               'again, or pass stale_ok=True to score the items as of the snapshot')

    def _snapshot_P(self, snap: CatalogueSnapshot, sp) -> Tensor:
        """the items' half of fc1 (tg_rank_cand_half), computed once per state of the score head's parameters"""
        stamp = self._score_stamp()
        if snap._P is None or snap._P_stamp != stamp:
            P = torch.empty_like(snap.h)
            check(lib.tg_rank_cand_half(len(snap), self.memory_dim, self.n_neighbors, C.byref(sp), ptr(snap.h), ptr(P),
                                        stream_ptr(self.device)), 'tg_rank_cand_half')
            snap._P, snap._P_stamp = P, stamp
        return snap._P

    def recommend(self, src_ids: Tensor, ts: Tensor, cand: Union[Tensor, CatalogueSnapshot], k: int, *,
                  mask: Optional[Tensor] = None, exclude_seen: bool = False, graph=None, chunk_queries: int = 65536,
                  col_of: Optional[Tensor] = None, uptodate: Optional[Tensor] = None,
                  catalogue_at: Optional[float] = None, stale_ok: bool = False):
        """The k best destinations of every (source, time) query among its candidates, on the model's CURRENT state,
        writing nothing -> (ids int64 [B, k], scores float32 [B, k], n_valid int32 [B]).  cand: int64 [B, C], or [C]
        shared by all queries (a catalogue).  A candidate is left out when it is the padding id 0, when mask[i, j] is false
        (mask: bool [B, C], or [C] with a shared catalogue), or - exclude_seen=True, shared catalogue only - when the
        source has an edge with it before ts[i] in `graph` (tg_seen_mask; col_of: `hip_ops.catalogue_index(cand, n_nodes)`
        when the caller has it, built here otherwise).  Order: higher score first, equal scores in the candidates'
        order (tg_topk_rows); positions past n_valid[i] hold id 0 and score -inf.  The scores are those of rank_scores
        (the same pair scores through `_pair_scores`, so a pair's bits do not depend on where it stands); queries run in
        chunks of at most `chunk_queries` pair scores.  A non-finite score among the candidates left in raises ValueError.
        Refused before anything runs: whatever rank_scores refuses (strategy 'uniform', a partitioned model, training
        mode, unaligned 'vec' hits); exclude_seen with per-query candidates.
        uptodate (a bitmap of hip_ops.new_bitmap; TIGER only): lazy restarts, as in rank_scores - this form WRITES
        MEMORIES: before the first chunk is scored, ONE `restart_involved` over the B (1 + C) queries (sources, then every
        query's candidates at its time) restarts what the bitmap does not hold yet and marks it; `last_restarted` holds
        the count.  A process that has loaded a checkpoint and a graph can answer without replaying the stream: memories
        at reset, an empty bitmap.
        Catalogue snapshots.  cand may be a CatalogueSnapshot (embed_catalogue): the items were embedded once, at the
        snapshot's time t, and are not embedded again.  Only the B sources are embedded, at their own ts[i]; the scores
        come from tg_rank_scores_shared - the items' half of the score head once per item, O(d) work per pair - and mask,
        exclude_seen, col_of, the chunking and the non-finite check work as above.  When every ts[i] equals t the lists
        are those of the tensor form bit for bit; for ts[i] > t they are the serving approximation "items as of the
        snapshot": an item's embedding and neighbour list are those of time t, never of a query's future.
        catalogue_at=t with a tensor cand [C] is the one-shot form: a snapshot is built at t, used and dropped; with
        `uptodate`, ONE `restart_involved` over the B + C queries [(src[i], ts[i]) ..., (cand[j], t) ...] runs before
        anything is embedded.  stale_ok=True uses a snapshot although the state, the parameters or the graph have changed
        since it was embedded: items as of the snapshot.  Refused before anything runs, with state and bitmap untouched:
        ts[i] < t for some i (the snapshot would come from that query's future); a snapshot of another model, device or
        graph size; a stale snapshot (RuntimeError) unless stale_ok; `uptodate` together with a ready snapshot (the
        restart would make it stale); catalogue_at with per-query candidates [B, C] or with a snapshot; 'vec' hits with
        an odd memory_dim.
        `recommend_subset` ranks per-query candidates on a snapshot's rows."""
        return self._recommend(src_ids, ts, cand, k, mask, exclude_seen, graph, chunk_queries, col_of, uptodate, catalogue_at,
                               stale_ok, None)

    def recommend_subset(self, src_ids: Tensor, ts: Tensor, cand: Union[Tensor, CatalogueSnapshot], k: int, subset: Tensor, *,
                         mask: Optional[Tensor] = None, graph=None, chunk_queries: int = 65536,
                         uptodate: Optional[Tensor] = None, catalogue_at: Optional[float] = None, stale_ok: bool = False):
        """Retrieve, then rank on a catalogue snapshot: `recommend` with every query ranking its OWN candidates `subset`
        (int64 [B, Cq] node ids, e.g. the ids of `hip_ops.walk_candidates`) on the snapshot's rows -> the 3-tuple of
        recommend.  cand: a CatalogueSnapshot, or a tensor catalogue [C] with catalogue_at=t (the one-shot form; with
        `uptodate` ONE `restart_involved` over the B + C queries, as in recommend).  col = snapshot.col_of[subset] names
        each candidate's row; a candidate is left out when it is not in the catalogue (col < 0), when it is the padding
        id 0 or when mask[i, q] is false (mask: bool [B, Cq]).  Only the B sources are embedded; the scores come from
        tg_rank_scores_gathered - one gathered row of P and O(d) work per pair, the bits of tg_rank_scores_shared at
        [i, col] - in chunks of chunk_queries // (Cq + 1) queries, and the returned ids are subset's.  With every
        ts[i] == t and every id in the catalogue the lists are those of recommend(src, ts, subset, k) bit for bit.
        There is no exclude_seen: that filter works on catalogue columns and would rebuild [B, C]; filter where the subset
        is generated (walk_candidates(exclude_seen=True)), as for per-query candidates.  Refused before anything runs,
        with state and bitmap untouched: a cand that is neither a snapshot nor a catalogue with catalogue_at, a subset of
        another shape than [B, Cq], an id outside [0, n_nodes), a catalogue that lists an id twice (its rows cannot be
        named by id), and everything recommend on a snapshot refuses."""
        if subset is None:
            raise ValueError('recommend_subset: subset is int64 [B, Cq]; without one, call recommend')
        return self._recommend(src_ids, ts, cand, k, mask, False, graph, chunk_queries, None, uptodate, catalogue_at, stale_ok,
                               subset)

    def _snapshot_scores(self, snap: CatalogueSnapshot, P: Tensor, sp, src_c: Tensor, h_src: Tensor,
                         nb_src: Optional[Tensor], col: Optional[Tensor] = None) -> Tensor:
        """one score block of a chunk's b sources (ids src_c, rows h_src / nb_src of `_embed_queries`) on the snapshot's
        rows, whose item half is P: float32 [b, C] over all C rows (tg_rank_scores_shared), or, with col int32 [b, Cq]
        naming a snapshot row per pair (-1: not in the catalogue), [b, Cq] (tg_rank_scores_gathered)"""
        d, K, dev = self.memory_dim, self.n_neighbors, self.device
        b, Cc = src_c.numel(), snap.ids.numel()
        with torch.no_grad():
            scores = torch.empty(b, Cc if col is None else col.shape[1], dtype=torch.float32, device=dev)
            if col is None:
                ws = self._ws('rank', int(lib.tg_rank_scores_shared_workspace_bytes(b, d, C.byref(sp))))
                check(lib.tg_rank_scores_shared(b, Cc, d, K, C.byref(sp), ptr(h_src), ptr(P), ptr(nb_src), ptr(snap.nb),
                                                ptr(src_c), ptr(snap.ids), ptr(scores), Cc, ptr(ws), ws.numel(),
                                                stream_ptr(dev)), 'tg_rank_scores_shared')
            else:
                ws = self._ws('rank', int(lib.tg_rank_scores_gathered_workspace_bytes(b, d, C.byref(sp))))
                check(lib.tg_rank_scores_gathered(b, Cc, col.shape[1], d, K, C.byref(sp), ptr(h_src), ptr(P), ptr(nb_src),
                                                  ptr(snap.nb), ptr(src_c), ptr(snap.ids), ptr(col), ptr(scores),
                                                  col.shape[1], ptr(ws), ws.numel(), stream_ptr(dev)),
                      'tg_rank_scores_gathered')
        return scores

    def _recommend(self, src_ids, ts, cand, k, mask, exclude_seen, graph, chunk_queries, col_of, uptodate, catalogue_at,
                   stale_ok, subset):
        """the body of recommend (subset None) and recommend_subset"""
        graph, strategy = self._pair_refusals('recommend', graph, chunk_queries, uptodate)
        dev = self.device
        snap = cand if isinstance(cand, CatalogueSnapshot) else None
        if snap is not None:
            if catalogue_at is not None:
                raise ValueError('recommend: catalogue_at builds a snapshot from a tensor cand [C]; cand is a snapshot already')
            if uptodate is not None:
                raise ValueError('recommend: uptodate with a ready catalogue snapshot - the restart would make the snapshot '
                                 'stale.  Either pass the catalogue as a tensor with catalogue_at=t (the one-shot form: one '
                                 'restart over sources and items, then the snapshot), or run restart_involved on the '
                                 'sources first and then embed_catalogue(..., uptodate=bitmap)')
            self._check_snapshot(snap, graph, stale_ok)
            cand = snap.ids
        if snap is not None or catalogue_at is not None:
            self._shared_refusals('recommend')
        src_ids = src_ids.to(dev).long().contiguous().reshape(-1)
        cand = torch.as_tensor(cand).to(dev).long().contiguous()
        B, k = src_ids.numel(), int(k)
        shared = cand.dim() == 1
        if not 1 <= k <= TG_TOPK_MAX_K:
            raise ValueError(f'recommend: 1 <= k <= {TG_TOPK_MAX_K}')
        if cand.dim() not in (1, 2) or (not shared and cand.shape[0] != B) or ts.numel() != B:
            raise ValueError(f'recommend: {B} queries, ts {tuple(ts.shape)}, cand {tuple(cand.shape)}')
        if exclude_seen and not shared:
            raise ValueError('recommend: exclude_seen needs a shared catalogue cand [C]')
        if catalogue_at is not None and not shared:
            raise ValueError('recommend: catalogue_at needs a shared catalogue cand [C], not per-query candidates [B, C]')
        Cc = cand.shape[-1]
        if subset is not None:
            if snap is None and catalogue_at is None:
                raise ValueError('recommend: subset ranks per-query candidates on the rows of a catalogue snapshot; give a '
                                 'snapshot, or a catalogue cand [C] with catalogue_at=t')
            subset = torch.as_tensor(subset).to(dev).long().contiguous()
            if subset.dim() != 2 or subset.shape[0] != B:
                raise ValueError(f'recommend: subset {tuple(subset.shape)} for {B} queries; per-query candidates are int64 [B, Cq]')
            if subset.numel():
                self._check_ids(subset, 'recommend: a node id outside [0, n_nodes) in subset')
        Cq = Cc if subset is None else subset.shape[1]  # score columns per query
        if mask is not None:
            mask = torch.as_tensor(mask).to(dev).bool()
            if subset is not None:
                if mask.shape != (B, Cq):
                    raise ValueError(f'recommend: mask {tuple(mask.shape)} for subset {tuple(subset.shape)}')
            elif mask.shape != ((Cc,) if mask.dim() == 1 and shared else (B, Cc)):
                raise ValueError(f'recommend: mask {tuple(mask.shape)} for cand {tuple(cand.shape)} of {B} queries')
        if B and Cc:
            self._check_ids(torch.cat([src_ids, cand.reshape(-1)]), 'recommend: a node id outside [0, n_nodes)')
        sub_col = None
        if subset is not None:  # the snapshot row of every candidate, -1: not in the catalogue
            try:
                sub_col = (snap.col_of if snap is not None else hip_ops.catalogue_index(cand, self.n_nodes))[subset]
            except ValueError as e:
                raise ValueError(f'recommend: subset names the rows of the catalogue by node id ({e})') from None
        if exclude_seen and col_of is None:
            col_of = hip_ops.catalogue_index(cand, self.n_nodes)
        ts64 = ts.to(dev).double().contiguous().reshape(-1)
        t_snap = snap.t if snap is not None else (None if catalogue_at is None else float(catalogue_at))
        if t_snap is not None:
            if t_snap != t_snap:
                raise ValueError('recommend: catalogue_at is NaN')
            if B and not bool((ts64 >= t_snap).all()):
                raise ValueError(f'recommend: a query time before the catalogue snapshot\'s time {t_snap!r} - the snapshot '
                                 "would come from that query's future")
        out_ids = torch.zeros(B, k, dtype=torch.int64, device=dev)
        out_scores = torch.full((B, k), float('-inf'), dtype=torch.float32, device=dev)
        n_valid = torch.zeros(B, dtype=torch.int32, device=dev)
        if B == 0 or Cc == 0 or Cq == 0:
            return out_ids, out_scores, n_valid
        if uptodate is not None:
            if catalogue_at is not None:  # B + C queries, one call, before anything is embedded
                self.restart_involved(torch.cat([src_ids, cand]),
                                      torch.cat([ts64, torch.full((Cc,), t_snap, dtype=torch.float64, device=dev)]), uptodate,
                                      graph=graph)
            else:
                self._restart_pairs(src_ids, cand.unsqueeze(0).expand(B, -1) if shared else cand, ts64, uptodate, graph)
        if catalogue_at is not None:
            snap = self._make_snapshot(cand, t_snap, graph, strategy)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        step = max(1, int(chunk_queries) // (Cq + 1))
        if snap is not None:
            from .training import score_struct
            with torch.no_grad():
                self._embed_prepare()
                sp = score_struct(self)
                P = self._snapshot_P(snap, sp)
                # the B sources are embedded once for all chunks, at their own times (a query's bits do not depend on the
                # list it is embedded in); only the [b, C] score block is chunked
                err = hip_ops.new_err(dev)
                h_all, nb_all = self._embed_queries(src_ids, ts64, graph, strategy, err)
                hip_ops.raise_if_err(err)
        for lo in range(0, B, step):
            hi = min(B, lo + step)
            nb_c = None if snap is None or nb_all is None else nb_all[lo:hi]
            if subset is not None:  # a per-query subset of the snapshot's rows
                col_c = sub_col[lo:hi]
                scores = self._snapshot_scores(snap, P, sp, src_ids[lo:hi], h_all[lo:hi], nb_c, col_c)
                mk = col_c >= 0
                if mask is not None:
                    mk = mk & mask[lo:hi]
                top = hip_ops.topk_rows(scores, subset[lo:hi], k, mask=mk, acc=bad)
                out_ids[lo:hi], out_scores[lo:hi], n_valid[lo:hi] = top['ids'], top['scores'], top['n_valid']
                continue
            ids = cand.unsqueeze(0).expand(hi - lo, -1) if shared else cand[lo:hi]
            if snap is None:
                scores = self._pair_scores('recommend', src_ids[lo:hi], ids, ts64[lo:hi], graph, strategy, chunk_queries)
            else:  # the items' rows are the snapshot's
                scores = self._snapshot_scores(snap, P, sp, src_ids[lo:hi], h_all[lo:hi], nb_c)
            mk = None
            if mask is not None:
                mk = mask.unsqueeze(0).expand(hi - lo, -1) if mask.dim() == 1 else mask[lo:hi]
            if exclude_seen:
                mk = hip_ops.seen_mask(graph, src_ids[lo:hi], ts64[lo:hi], col_of, Cc, mask=mk)
            top = hip_ops.topk_rows(scores, cand if shared else ids, k, mask=mk, acc=bad)
            out_ids[lo:hi], out_scores[lo:hi], n_valid[lo:hi] = top['ids'], top['scores'], top['n_valid']
        n_bad = int(bad.item())
        if n_bad:
            raise ValueError(f'Input contains {n_bad} non-finite scores.')
        return out_ids, out_scores, n_valid

    def recommend_walk(self, src_ids: Tensor, ts: Tensor, k: int, *, C: int = 256, graph=None,
                       uptodate: Optional[Tensor] = None, chunk_queries: int = 65536,
                       snapshot: Optional[CatalogueSnapshot] = None, fill: Optional[dict] = None, **walk):
        """Retrieve, then rank: every query's candidates come from the graph itself - `hip_ops.walk_candidates` over the
        graph `recommend` would use, at the query's own time, C per query (**walk: its fanout / take / exclude_seen /
        keep_self) - and `recommend` lists the k best of them -> (ids int64 [B, k], scores float32 [B, k], n_valid int32
        [B], cand: the dict of walk_candidates).  Exactly `recommend(src_ids, ts, cand['ids'], k, ...)`: the per-query form
        drops the padding id 0, `uptodate` restarts what the B (1 + C) queries involve, and whatever `recommend` refuses
        is refused here before the walk runs.  The walk's own exclude_seen is the seen-item filter of this form.
        snapshot (a CatalogueSnapshot of embed_catalogue): the candidates are ranked on the snapshot's rows instead of
        being embedded - exactly `recommend_subset(src_ids, ts, snapshot, k, cand['ids'])`: B source
        embeddings and one gathered pair score per candidate; a candidate that is not in the catalogue is left out.
        cand then also holds n_in_catalogue int32 [B], the valid candidates of each query that the catalogue lists.
        `uptodate` together with a snapshot is refused as in recommend.
        fill=dict(T=..., window=None, among=None, t=None): back-fill the rows the walk leaves short with what is popular
        right now - `hip_ops.trending` ONCE per call (the T most active nodes of [t - window, t); t defaults to the earliest
        query time, so nothing comes from any query's future; among defaults to snapshot.ids with a snapshot, else to all
        nodes), then `hip_ops.fill_candidates` under the walk's own exclude_seen / keep_self, then the ranking above on the
        filled rows.  cand is then the filled dict: its counts are 0 in the filled columns and it gains n_filled int32 [B].
        A source without entries gets the trending list.  fill=None is the path above, unchanged."""
        graph, _ = self._pair_refusals('recommend_walk', graph, chunk_queries, uptodate)
        if fill is not None:
            fill = hip_ops._fill_plan('recommend_walk', fill)
        if not 1 <= int(k) <= TG_TOPK_MAX_K:
            raise ValueError(f'recommend_walk: 1 <= k <= {TG_TOPK_MAX_K}')
        if snapshot is not None:
            if not isinstance(snapshot, CatalogueSnapshot):
                raise ValueError('recommend_walk: snapshot is a CatalogueSnapshot of embed_catalogue')
            if uptodate is not None:
                raise ValueError('recommend_walk: uptodate with a ready catalogue snapshot - the restart would make the '
                                 'snapshot stale.  Run restart_involved on the sources first, then '
                                 'embed_catalogue(..., uptodate=bitmap)')
            self._check_snapshot(snapshot, graph, False)
        dev = self.device
        src_ids = src_ids.to(dev).long().contiguous().reshape(-1)
        ts64 = ts.to(dev).double().contiguous().reshape(-1)
        cand = hip_ops.walk_candidates(graph, src_ids, ts64, C, **walk)
        if fill is not None and src_ids.numel():
            among = fill['among'] if fill['among'] is not None else (snapshot.ids if snapshot is not None else None)
            if among is not None:
                among = torch.as_tensor(among).to(dev)
            t0 = float(ts64.min()) if fill['t'] is None else float(fill['t'])
            trend = hip_ops.trending(graph, t0, fill['T'], window=fill['window'], among=among)
            cand = hip_ops.fill_candidates(graph, src_ids, ts64, cand, trend, exclude_seen=bool(walk.get('exclude_seen', False)),
                                           keep_self=bool(walk.get('keep_self', False)))
        elif fill is not None:
            cand['n_filled'] = torch.zeros(0, dtype=torch.int32, device=dev)
        if snapshot is None:
            ids, scores, n_valid = self.recommend(src_ids, ts64, cand['ids'], k, graph=graph, chunk_queries=chunk_queries,
                                                  uptodate=uptodate)
        else:
            ids, scores, n_valid = self.recommend_subset(src_ids, ts64, snapshot, k, cand['ids'], graph=graph,
                                                         chunk_queries=chunk_queries)
            found = (snapshot.col_of[cand['ids']] >= 0) & (cand['ids'] != 0)
            cand['n_in_catalogue'] = found.sum(1).to(torch.int32)
        return ids, scores, n_valid, cand

    # ---- embedding nearest neighbours on a catalogue snapshot ----------------------------------------------
    def _similar_refusals(self, what: str, snapshot, graph, stale_ok: bool, metric: str):
        self._refuse_partitioned(what)
        if not isinstance(snapshot, CatalogueSnapshot):
            raise ValueError(f'{what}: snapshot is a CatalogueSnapshot of embed_catalogue')
        if metric not in ('cos', 'ip'):
            raise ValueError(f"{what}: metric is 'cos' or 'ip', got {metric!r}")
        self._check_snapshot(snapshot, self.graph if graph is None else graph, stale_ok)

    def _similar(self, what: str, items: Tensor, snapshot: CatalogueSnapshot, k: int, metric: str, exclude_self: bool,
                 mask: Optional[Tensor], found: Optional[Tensor] = None) -> dict:
        """tg_knn_rows of the snapshot rows of `items` against all rows -> the dict of hip_ops.knn_rows.  found (bool [B]):
        the items that have a row; the others get an empty list (n_valid 0, padding) instead of being refused"""
        dev = self.device
        col = snapshot.col_of[items].long()
        if found is not None:
            col = torch.where(found, col, torch.zeros_like(col))
        q = snapshot.h[col]
        cos = metric == 'cos'
        inv = snapshot.inv_norm if cos else None
        if mask is not None:
            mask = torch.as_tensor(mask).to(dev)
            if mask.dtype != torch.bool or mask.shape != (len(snapshot),):
                raise ValueError(f'{what}: mask is bool [C = {len(snapshot)}], got {mask.dtype} {tuple(mask.shape)}')
        out = hip_ops.knn_rows(q, snapshot.h, k, ids=snapshot.ids, q_scale=inv[col] if cos else None, c_scale=inv,
                               exclude=items if exclude_self else None, col_mask=mask)
        if found is not None and items.numel():
            lost = ~found
            out['ids'][lost] = 0
            out['scores'][lost] = float('-inf')
            out['cols'][lost] = -1
            out['n_valid'][lost] = 0
        return out

    @torch.no_grad()
    def similar_items(self, items: Tensor, snapshot: CatalogueSnapshot, k: int, *, metric: str = 'cos',
                      exclude_self: bool = True, mask: Optional[Tensor] = None, stale_ok: bool = False):
        """The k nearest catalogue items of every item in embedding space, both "as of the snapshot": the query rows are
        snapshot.h[snapshot.col_of[items]], the catalogue is snapshot.h, and tg_knn_rows selects on the MFMA accumulators -
        the [B, C] matrix is never formed -> (ids int64 [B, k], scores float32 [B, k], n_valid int32 [B]).  metric 'ip': the
        float32 inner product (the fmaf chain of tiger_hip.h); 'cos': that times snapshot.inv_norm of the item, then of the
        neighbour (a zero row scores 0 against everything).  exclude_self leaves the item itself out of its own list; mask:
        bool [C] over the snapshot's rows, false = left out for every item.  Padding id 0 rows of the snapshot and
        non-finite scores are left out; order and padding are those of recommend (tg_topk_rows).  Reads nothing but the
        snapshot, writes nothing.  Refused before anything runs: what recommend on a snapshot refuses (another model's or
        device's snapshot, a stale one - RuntimeError - unless stale_ok; a partitioned model); an item that is the
        padding id 0, outside [0, n_nodes) or not in the snapshot, naming the first offender; k outside
        [1, TG_TOPK_MAX_K]; a memory_dim that tg_knn_rows does not take (a multiple of 4, at most 512)."""
        self._similar_refusals('similar_items', snapshot, None, stale_ok, metric)
        items = torch.as_tensor(items).to(self.device).long().contiguous().reshape(-1)
        if not 1 <= int(k) <= TG_TOPK_MAX_K:
            raise ValueError(f'similar_items: 1 <= k <= {TG_TOPK_MAX_K}')
        if items.numel():
            bad = (items <= 0) | (items >= snapshot.col_of.numel())
            bad = bad | (snapshot.col_of[torch.where(bad, torch.zeros_like(items), items)] < 0)
            if bool(bad.any()):
                at = int(bad.int().argmax())
                raise ValueError(f'similar_items: item {int(items[at])} (position {at}) is the padding id 0, outside '
                                 f'[0, {self.n_nodes}) or not in the snapshot')
        out = self._similar('similar_items', items, snapshot, int(k), metric, exclude_self, mask)
        return out['ids'], out['scores'], out['n_valid']

    def similar_items_keys(self, idmap, item_keys, snapshot: CatalogueSnapshot, k: int, **kw):
        """`similar_items` behind external keys -> (keys int64 [B, k], scores, n_valid); keys = idmap.keys_of(ids), so
        positions past n_valid[i] hold INT64_MIN, as in recommend_keys.  A key the map (or the model) does not know raises
        ValueError saying how many."""
        item_keys = self._device_keys('similar_items_keys', 'item_keys', item_keys).reshape(-1)
        if idmap.device != self.device:
            raise ValueError(f'similar_items_keys: the id map lives on {idmap.device}, the model on {self.device}')
        ids = idmap.lookup(item_keys)
        unknown = int(((ids < 0) | (ids >= self.n_nodes)).sum())
        if unknown:
            raise ValueError(f'similar_items_keys: {unknown} of the {ids.numel()} items are keys the model has never seen')
        out, scores, n_valid = self.similar_items(ids.long(), snapshot, k, **kw)
        return idmap.keys_of(out, check=False), scores, n_valid

    def recommend_similar(self, src_ids: Tensor, ts: Tensor, snapshot: CatalogueSnapshot, k: int, *, S: int = 64,
                          seeds: Optional[Tensor] = None, metric: str = 'cos', graph=None, **recommend_subset_kwargs):
        """Retrieve in embedding space, rank with the score head: every query's candidates are the S nearest snapshot rows
        of its SEED item (`similar_items` without the seed itself), and `recommend_subset(src_ids, ts, snapshot, k,
        cand['ids'])` lists the k best of them -> (ids int64 [B, k], scores float32 [B, k], n_valid int32 [B], cand =
        dict(ids int64 [B, S], scores, cols, n_valid, seeds)).  seeds: int64 [B], 0 = none; None: each source's latest
        neighbour strictly before its time, `hip_ops.walk_candidates(graph, src, ts, 1, fanout=(1,), take=(True,))`.  A
        query whose seed is 0 or not in the snapshot has no candidates: n_valid == 0.  S <= TG_TOPK_MAX_K (tg_knn_rows
        selects at most that many; a larger S is refused, not looped).
        The approximation is recommend_subset's: items as of the snapshot - seed and neighbours are the snapshot's rows,
        never a query's future.  Inner-product or cosine nearness of embeddings is NOT what the score head was trained on:
        the generator proposes, the score head disposes, and the effect of this generator on hit rate / NDCG with trained
        weights has not been measured.  Whatever recommend_subset refuses is refused before the retrieval runs."""
        graph, _ = self._pair_refusals('recommend_similar', graph, int(recommend_subset_kwargs.get('chunk_queries', 65536)),
                                       recommend_subset_kwargs.get('uptodate'))
        if not 1 <= int(S) <= TG_TOPK_MAX_K:
            raise ValueError(f'recommend_similar: 1 <= S <= {TG_TOPK_MAX_K} (TG_TOPK_MAX_K, the most positions tg_knn_rows '
                             'selects per row)')
        if not 1 <= int(k) <= TG_TOPK_MAX_K:
            raise ValueError(f'recommend_similar: 1 <= k <= {TG_TOPK_MAX_K}')
        self._similar_refusals('recommend_similar', snapshot, graph, bool(recommend_subset_kwargs.get('stale_ok', False)), metric)
        self._shared_refusals('recommend_similar')
        dev = self.device
        src_ids = src_ids.to(dev).long().contiguous().reshape(-1)
        ts64 = ts.to(dev).double().contiguous().reshape(-1)
        B = src_ids.numel()
        if ts64.numel() != B:
            raise ValueError(f'recommend_similar: {B} queries, ts {tuple(ts.shape)}')
        if seeds is None:
            seeds = hip_ops.walk_candidates(graph, src_ids, ts64, 1, fanout=(1,), take=(True,))['ids'].reshape(-1)
        else:
            seeds = torch.as_tensor(seeds).to(dev).long().contiguous().reshape(-1)
            if seeds.numel() != B:
                raise ValueError(f'recommend_similar: {B} queries, seeds {tuple(seeds.shape)}')
            if B:
                self._check_ids(seeds, 'recommend_similar: a seed outside [0, n_nodes)')
        with torch.no_grad():
            col_of = snapshot.col_of
            found = (seeds > 0) & (col_of[seeds.clamp(0, col_of.numel() - 1)] >= 0) if B else seeds.bool()
            cand = self._similar('recommend_similar', seeds, snapshot, int(S), metric, True, None, found)
        cand['seeds'] = seeds
        ids, scores, n_valid = self.recommend_subset(src_ids, ts64, snapshot, k, cand['ids'], graph=graph,
                                                     **recommend_subset_kwargs)
        return ids, scores, n_valid, cand

    # ---- fused path ---------------------------------------------------------------------
    class StepBuffers:
        """Static device buffers of one batch size: inputs, outputs and the workspace of
        tg_stream_step; reused every step so the call sequence can be graph-captured."""

        def __init__(self, model: 'TIGE', B: int, want_prev: bool, resident=None, embed_only: bool = False,
                     h_out=None, h_new_out=None, want_h_new: bool = True, lean: bool = False, prefetch: bool = False,
                     debug_lists: bool = False, collate_only: bool = False):
            """resident = (src, dst, neg, ts64, eids) device tensors of the WHOLE stream: the
            step then reads batch [offset, offset+B) and advances `offset` on device.
            lean: the caller does not read `involved` nor counts[0:2] (tiger_hip.h: tg_step_io.lean) - an eager
            step then skips forming those sets; same results otherwise.
            prefetch (resident streams): the caller does not read the neighbour lists either (l1_* are not outputs then) - a
            lean eager step of a model with eager query rows then runs the NEXT batch's sampler and centres as riders of its
            own last launch (tiger_hip.h: tg_step_io.prefetch_state); same results otherwise.
            collate_only: buffers of a collate-only pass (tg_step_io.collate_only; the caller sets the flag): no embedding rows,
            the lists and the involved set stay in the workspace - a third of the allocations (a restart-mode evaluation
            pass builds sixteen such contexts)."""
            dev, d, K = model.device, model.memory_dim, model.n_neighbors
            self.B = B
            self.embed_only = embed_only
            i64 = dict(dtype=torch.int64, device=dev)
            self.offset = None
            if resident is None:
                self.src, self.dst, self.neg, self.eids = (torch.zeros(B, **i64) for _ in range(4))
                self.ts = torch.zeros(B, dtype=torch.float64, device=dev)
            else:
                self.src, self.dst, self.neg, self.ts, self.eids = resident
                assert self.ts.dtype == torch.float64 and all(t.is_contiguous() for t in resident)
                self.offset = torch.zeros(1, **i64)
            # h_out / h_new_out: caller-owned output rows (e.g. slices of an all-gather send buffer)
            if collate_only:
                self.h = self.l1_nids = self.l1_eids = self.l1_ts = self.involved = None
                want_prev = want_h_new = False
            else:
                self.h = h_out if h_out is not None else torch.zeros(3 * B, d, dtype=torch.float32, device=dev)
                self.l1_nids = torch.zeros(3 * B, K, **i64)
                self.l1_eids = torch.zeros(3 * B, K, **i64)
                self.l1_ts = torch.zeros(3 * B, K, dtype=torch.float32, device=dev)
                self.involved = torch.zeros(3 * B * (K + 1), **i64)
            self.counts = torch.zeros(4, dtype=torch.int32, device=dev)
            self.err = torch.zeros(1, dtype=torch.int32, device=dev)
            self.h_prev_left = torch.zeros(2 * B, d, dtype=torch.float32, device=dev) if want_prev else None
            self.h_prev_right = torch.zeros(2 * B, d, dtype=torch.float32, device=dev) if want_prev else None
            self.h_new = h_new_out if h_new_out is not None else (
                torch.zeros(2 * B, d, dtype=torch.float32, device=dev) if (embed_only and want_h_new) else None)
            m = model.model_struct()
            nbytes = int(lib.tg_stream_step_workspace_bytes2(C.byref(m), B, model.n_layers))
            if nbytes == 0:
                raise RuntimeError('tg_stream_step: unsupported model dimensions')
            self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # zero-filled: the step keeps it clean
            self.io = TgStepIo(B, ptr(self.src), ptr(self.dst), ptr(self.neg), ptr(self.ts), ptr(self.eids),
                               ptr(self.h), ptr(self.l1_nids), ptr(self.l1_eids), ptr(self.l1_ts), ptr(self.involved),
                               ptr(self.counts), ptr(self.h_prev_left), ptr(self.h_prev_right), ptr(self.err),
                               ptr(self.offset), 1 if resident is not None else 0, 1 if embed_only else 0, None,
                               ptr(self.h_new), 0 if embed_only else 1, 0)
            self.io.lean = 1 if lean else 0
            # collate prefetch (tiger_hip.h: tg_step_io.prefetch_state): a lean step over a resident stream runs the next
            # batch's sampler + centres on its own last launch; TIGE.launch_step keeps the promise the flag stands for
            self._pf_state = C.c_int32(0)
            self._pf_stamp = None
            if prefetch:
                if resident is None or embed_only:
                    raise ValueError('prefetch needs a resident stream and a full step')
                self.io.stream_len = int(self.src.numel())
                self.io.prefetch_state = C.addressof(self._pf_state)
                self.io.l1_nids = self.io.l1_eids = self.io.l1_ts = None
            # debug_lists: the neighbour lists of the batch a step CONSUMES, copied out before its last launch replaces them
            # (tiger_hip.h: tg_step_io.dbg_l1_*) - the collate-prefetch form has no other way to show them
            self.dbg_l1_nids = self.dbg_l1_eids = self.dbg_l1_ts = None
            if debug_lists:
                self.dbg_l1_nids = torch.zeros(3 * B, K, **i64)
                self.dbg_l1_eids = torch.zeros(3 * B, K, **i64)
                self.dbg_l1_ts = torch.zeros(3 * B, K, dtype=torch.float32, device=dev)
                self.io.dbg_l1_nids, self.io.dbg_l1_eids, self.io.dbg_l1_ts = (ptr(self.dbg_l1_nids), ptr(self.dbg_l1_eids),
                                                                               ptr(self.dbg_l1_ts))

        def attach_profiler(self, prof):
            self.io.profiler = prof

        def enable_lazy_restart(self, model: 'TIGER', trigger, force_list: bool = False):
            """The lazy-restart loop of train_self_supervised.py:152-163 inside the step (static restarter only;
            tiger_hip.h: tg_lazy_restart).  trigger[b] != 0 means the reference's `np.random.rand() < restart_prob`
            fired before batch b (the loop never fires before batch 0); the draws are the caller's, made up front,
            so a run is reproducible and the step stays free of host round trips.  counts[3] of every step is the
            number of nodes re-initialised by it.  force_list: the list form below for the static restarter too (a caller
            that drives another step function than launch_step, e.g. the resident evaluation pass)."""
            from .restarters import StaticRestarter
            r = getattr(model, 'restarter_fn', None)
            if r is None:
                raise NotImplementedError('the lazy-restart loop needs a model with a restarter (TIGER)')
            dev = model.device
            self.lazy_trigger = torch.as_tensor(trigger).to(dev, torch.uint8).contiguous()
            self.lazy_batch = torch.zeros(1, dtype=torch.int64, device=dev)
            self.lazy_restarting = torch.zeros(1, dtype=torch.int32, device=dev)
            self.lazy_uptodate = torch.zeros(hip_ops.bitmap_words(model.n_nodes), dtype=torch.int64, device=dev)
            if isinstance(r, StaticRestarter) and not force_list:  # the whole loop body runs inside the step
                self._lazy = TgLazyRestart(ptr(r.left_emb.weight), ptr(r.right_emb.weight), ptr(self.lazy_trigger),
                                           self.lazy_trigger.numel(), ptr(self.lazy_batch), ptr(self.lazy_restarting),
                                           ptr(self.lazy_uptodate), None, None)
                self.io.lazy = C.addressof(self._lazy)
                return self
            # Any other restarter (the SeqRestarter of the reference's default recipe, init_utils.py:55-58): the LIST form.
            # The loop's bookkeeping - trigger, uptodate / has-message bitmaps, involved & ~uptodate - runs on the device in
            # a collate-only pass; the host reads back ONE count, runs restarter + tg_restart_apply on the device-resident
            # list and then launches the step (TIGE.launch_step).  No node list crosses the host link, no Python sets.
            self.lazy_restarted = 0  # nodes re-initialised before the last step (the step's own counts[3] stays 0)
            cb = self.lazy_collate_context(model)
            self.lazy_list, self.lazy_tmin, self._lazy = cb.lazy_list, cb.lazy_tmin, cb._lazy
            self._lazy_collate = cb
            self._lazy_host = torch.zeros(2, dtype=torch.float32).pin_memory() if dev.type == 'cuda' else None
            return self

        def lazy_collate_context(self, model: 'TIGER'):
            """One collate-only pass of the list form (see enable_lazy_restart): step buffers of its own, its own list /
            earliest-time / count outputs, the loop variables (trigger, batch counter, restarting flag, up-to-date bitmap) of
            THIS buffer.  By default it reads the batch at this buffer's device-side offset without advancing it; a caller
            that runs passes ahead of the steps (eval_utils: the resident restart-mode pass) points `io.offset_dev` elsewhere."""
            dev = model.device
            cap = min(3 * self.B * (model.n_neighbors + 1), model.n_nodes)
            cb = TIGE.StepBuffers(model, self.B, False, resident=(self.src, self.dst, self.neg, self.ts, self.eids),
                                  collate_only=True)
            cb.lazy_list = torch.zeros(max(cap, 1), dtype=torch.int64, device=dev)
            cb.lazy_tmin = torch.zeros(1, dtype=torch.float32, device=dev)
            cb._lazy = TgLazyRestart(None, None, ptr(self.lazy_trigger), self.lazy_trigger.numel(), ptr(self.lazy_batch),
                                     ptr(self.lazy_restarting), ptr(self.lazy_uptodate), ptr(cb.lazy_list), ptr(cb.lazy_tmin))
            if self.offset is not None:  # the same batch as the step that follows: its device-side offset, not advanced
                cb.offset = self.offset
                cb.io.offset_dev = ptr(self.offset)
            cb.io.advance = 0
            cb.io.collate_only = 1
            cb.io.lazy = C.addressof(cb._lazy)
            return cb

        def load(self, src, dst, neg, ts, eids):
            self.src.copy_(src, non_blocking=True)
            self.dst.copy_(dst, non_blocking=True)
            self.neg.copy_(neg, non_blocking=True)
            self.ts.copy_(ts, non_blocking=True)
            self.eids.copy_(eids, non_blocking=True)

    def step_buffers(self, B: int, want_prev: bool = False, lean: bool = False) -> 'TIGE.StepBuffers':
        key = ('step', B, want_prev, lean)
        buf = self._step_ws.get(key)
        if buf is None:
            buf = TIGE.StepBuffers(self, B, want_prev, lean=lean)
            self._step_ws[key] = buf
        return buf

    def check_graph(self, graph):
        """the tables of the model and the bitmaps of a step are indexed by node id: a graph over fewer ids (e.g.
        Graph.from_data(train_data) when the training split lacks the highest ids) must be built with
        max_node_id = the largest id of the full data"""
        if graph.num_node != self.n_nodes:
            raise ValueError(f'graph covers {graph.num_node} node ids, the model {self.n_nodes}: build every graph with '
                             'max_node_id = the largest node id of the full data (init_utils.init_data does)')

    def prepare_pass(self, cb: 'TIGE.StepBuffers', graph=None):
        """A collate-only pass (StepBuffers.lazy_collate_context) must flag exactly what the step will involve: it samples with
        the graph's own strategy and, on a two-layer model, both hops (data_loader.py:105-131: `np_computation_graph_nodes`
        holds the nodes of every layer).  Call before each pass (the structs carry pointers that follow the model)."""
        strategy = getattr(self.graph if graph is None else graph, 'strategy', 'recent_edges')
        cb.io.strategy = {'recent_edges': 0, 'recent_nodes': 1, 'uniform': 2}.get(strategy, 0)
        if self.n_layers == 2:
            cb._inner = self.model_struct(1)
            cb.io.inner = C.addressof(cb._inner)

    def rows_bound(self) -> int:
        """Bound on the nodes with a pending message per batch handed to the library (tg_step_io.rows_hint):
        1.5 x the largest count read back so far, 0 while nothing has been read back.  Performance only - but a
        launch sized for one round that needs a second one costs more than the smaller blocks win, and the count
        grows while the graph behind the stream fills up (C2: 3200 at batch 20, 4550 at batch 120), hence the
        generous margin; the bound follows the counts as they are read back."""
        if self._pending is not None:  # eager updates: the updater runs on the unique positive nodes of a batch
            # (their count barely moves from batch to batch - C2: 1 040 .. 1 070 - and the updater kernels this selects
            # size their blocks from the LIVE count: a batch above the bound costs that batch some speed, nothing else)
            seen = getattr(self, '_pos_seen', 0)
            return int(1.03 * seen) + 1 if seen else 0
        seen = getattr(self, '_rows_seen', 0)
        return int(1.5 * seen) + 64 if seen else 0

    def note_rows(self, n_outdated: int, n_unique_pos: int = 0):
        self._rows_seen = max(getattr(self, '_rows_seen', 0), int(n_outdated))
        self._pos_seen = max(getattr(self, '_pos_seen', 0), int(n_unique_pos))

    def launch_step(self, buf: 'TIGE.StepBuffers'):
        """Enqueue collate + STEP 1-6 for the batch already in `buf` (no host sync)."""
        if not (buf.embed_only or buf.io.collate_only):
            self._refuse_partitioned('stream_step / launch_step (a full step)')
        strategy = getattr(self.graph, 'strategy', 'recent_edges')
        if strategy not in ('recent_edges', 'recent_nodes', 'uniform'):
            raise NotImplementedError(f"the fused step samples 'recent_edges', 'recent_nodes' or 'uniform'; strategy={strategy!r} "
                                      '(graph.py:104-110, alpha != 0) is not built')
        buf.io.strategy = {'recent_edges': 0, 'recent_nodes': 1, 'uniform': 2}[strategy]
        if strategy == 'uniform':  # the graph's RandomState lives on the device and is consumed in query order
            buf.io.mt_state = ptr(self.graph._mt_state())
        if self.n_layers == 2:  # the second attention layer's weights travel in a tg_model of their own
            buf._inner = self.model_struct(1)
            buf.io.inner = C.addressof(buf._inner)
        buf.io.rows_hint = self.rows_bound()
        if self._fused is not None and self._fused_stamp != self._attn_stamp():
            # an attention parameter was updated in place since the weights were pre-multiplied (an optimizer step, a
            # copy_): recompute them instead of embedding with stale products
            if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('attention parameters changed since fuse_attention(): call it again before capturing')
            self.fuse_attention()
        self.check_graph(self.graph)
        g = self.graph.tcsr
        cb = getattr(buf, '_lazy_collate', None)
        if cb is not None:  # lazy-restart loop, list form (see StepBuffers.enable_lazy_restart)
            if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('the lazy-restart loop with a sequence restarter reads one count back per batch: '
                                   'it cannot be captured into a graph (the static restarter runs inside the step)')
            m = self.model_struct()
            self.prepare_pass(cb, self.graph)
            check(lib.tg_stream_step(C.byref(m), C.byref(g), C.byref(cb.io), ptr(cb.ws), cb.ws.numel(),
                                     stream_ptr(self.device)), 'tg_stream_step(lazy restart list)')
            n = int(cb.counts[3].item())  # the one read-back of the loop
            buf.lazy_restarted = n
            if n:
                self.restart(buf.lazy_list[:n], buf.lazy_tmin.expand(n))
            buf.lazy_batch += 1
        if self._pending is not None and not buf.embed_only:
            self._sync_pending()
            # the per-node tables: every step without the in-step restart loop reads them; one with the loop only in the form
            # the LIBRARY reports for this very call (tg_stream_step_form: lean, static restarter, centre-row table, no
            # h_prev outputs, no compact copy ... - its decision, not a restatement of it here)
            if not buf.io.lazy:
                self._sync_gtab()
            elif self._gtab_wanted():
                if getattr(self, '_gtab', None) is None:
                    self._sync_gtab()  # (allocates: the form is a function of the struct the step will see)
                if lib.tg_stream_step_form(C.byref(self.model_struct()), C.byref(buf.io)) & 8:
                    self._sync_gtab()
        m = self.model_struct()
        pf = bool(buf.io.prefetch_state)
        if pf:  # is the collate part this buffer's previous step prefetched still the one this step needs?
            # (a batch prefetched by a step of the four-launch form carries no pre-batch snapshot: only such a step may use
            # it.  The form is a function of the struct and the io fields as they stand now: asked once per step)
            defer = bool(lib.tg_stream_step_form(C.byref(m), C.byref(buf.io)) & TG_FORM_FC2_DEFERRED)
            lost_form = getattr(buf, '_pf_defer', False) and not defer
            if buf._pf_state.value == 1 and (buf._pf_stamp != self._prefetch_stamp(buf, g) or lost_form):
                if os.environ.get('TG_PF_DEBUG'):
                    print('prefetch discarded:', buf._pf_stamp, '->', self._prefetch_stamp(buf, g), flush=True)
                buf._pf_state.value = 2  # made, but for another state / offset / graph: the step discards it
            before = buf._pf_state.value
        self._step_serial = getattr(self, '_step_serial', 0) + 1
        if (self._tracker is not None or self._journal is not None) and not (buf.embed_only or buf.io.collate_only):
            self._mark_step(buf, buf.io)
        check(lib.tg_stream_step(C.byref(m), C.byref(g), C.byref(buf.io), ptr(buf.ws), buf.ws.numel(),
                                 stream_ptr(self.device)), 'tg_stream_step')
        if pf:
            if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                buf._pf_state.value = before  # nothing ran: the device is where it was before the capturing call
            buf._pf_stamp = self._prefetch_stamp(buf, g)
            buf._pf_defer = defer
        if (buf.io.lazy and getattr(self, '_gtab', None) is not None
                and not (lib.tg_stream_step_form(C.byref(m), C.byref(buf.io)) & 8)):
            self._gtab_stamp = None  # the in-step restart loop re-initialised rows the tables did not follow

    def _prefetch_stamp(self, buf, g):
        """Everything the prefetched collate part of a batch is a function of, as far as the host can see it: the state
        (as for the eager-update table), that no other step ran on this model since, the stream offset tensor and the
        graph.  (Graph replays change none of these: a graph captured with the flag set on entry and exit keeps it
        valid by construction.)"""
        # (the graph by its serial number too: the address of a dead graph's struct can be handed out again - Graph.extended)
        return (self._state_stamp(), getattr(self, '_step_serial', 0), buf.offset._version, id(buf.offset), C.addressof(g),
                getattr(g, 'serial', 0))

    @torch.no_grad()
    def stream_step(self, src, dst, neg, ts, eids, want_prev: bool = False, check_invariants: bool = True,
                    lean: bool = False):
        """Fused collate + STEP 1-6 (data_loader.py:77-131 + tiger.py:196-255).
        ts are the float64 event times.  Returns the StepBuffers (h = embeddings of
        cat[src,dst,neg]; rows [0,2B) are h_left).  lean: see StepBuffers."""
        dev = self.device
        to = lambda x, dt: torch.as_tensor(x).to(dev, dt)
        buf = self.step_buffers(len(src), want_prev, lean)
        buf.load(to(src, torch.int64), to(dst, torch.int64), to(neg, torch.int64), to(ts, torch.float64),
                 to(eids, torch.int64))
        self.launch_step(buf)
        if check_invariants:
            word = int(buf.err.item())
            cnt = buf.counts.tolist()
            self.note_rows(cnt[1], cnt[2])
            if word:
                buf.err.zero_()
                from .._lib import raise_invariants
                raise_invariants(word & 0xFFFFFFFF)
        return buf

    def observe(self, src, dst, ts, eids, *, efeats=None, neg=None, want_prev: bool = False, num_node=None, nfeats=None):
        """Online ingestion of one time-ordered batch of NEW events: their edge-feature rows (efeats [n, d_e], for a model
        with an edge table) are appended to the table, the graph is replaced by `graph.extended(...)` and the batch is
        streamed (`stream_step`; neg defaults to dst) -> the step's StepBuffers.  Extending first is what the reference's
        graph over the whole stream implies: an event sees same-batch events with a strictly earlier timestamp as
        neighbours.  A model that starts from a graph over a prefix of the stream and observes the rest ends in the state,
        and returns the embeddings, of a model that had the full graph from the start - bit for bit.  Afterwards
        `recommend(..., exclude_seen=True)` and `rank_scores` see the new edges.  eval() mode only; refused before anything
        runs: a partitioned model, training mode, an eid that is no row of the edge table (tg_model carries no row count:
        the step would read past the table), and what `Graph.extended` refuses.
        num_node: admit NEW NODE IDS with the batch.  An int N >= n_nodes, or 'auto' (= the batch's largest
        id + 1 when that is more than n_nodes): ids below N are accepted, the model's per-node tables grow to N rows
        (`grow_nodes`) and nfeats [N - n_nodes, d_n] become the feature rows of the ids [n_nodes, N) (zeros if omitted).
        A model built on N0 nodes that admits ids up to N1 on the way ends in the state, and returns the embeddings, of
        one built on N1 nodes - bit for bit.  The child graph is computed first (it validates), then what `grow_nodes`
        refuses is refused: nothing has changed if the call raises.  The caller's part is that of `grow_nodes`."""
        self._refuse_partitioned('observe')
        self._refuse_tracked('observe')
        if self.training:
            raise RuntimeError('observe streams the model in eval() mode')
        if num_node is None and nfeats is not None:
            raise ValueError('observe: nfeats are the feature rows of newly admitted node ids (pass num_node)')
        fg = self.raw_feat_getter
        n = len(src)
        if efeats is not None and fg.efeats is not None:
            efeats = torch.as_tensor(efeats)
            if efeats.dim() != 2 or efeats.shape[0] != n or efeats.shape[1] != fg.efeats.shape[1]:
                raise ValueError(f'observe: efeats {tuple(efeats.shape)} for {n} events of width {fg.efeats.shape[1]}')
        rows = None if fg.efeats is None else fg.efeats.shape[0] + (n if efeats is not None else 0)
        # (validates, the eids against the table's rows included - on the host, before any launch; nothing has changed if
        # it raises)
        if num_node is None:
            new_graph = self.graph.extended(src, dst, ts, eids, eid_rows=rows)
        else:
            new_graph = self.graph.extended(src, dst, ts, eids, eid_rows=rows, num_node=num_node)
            nfeats = self._grow_refusals('observe', max(new_graph.num_node, self.n_nodes), nfeats, None)
        if efeats is not None and fg.efeats is not None and fg.append_edge_rows(efeats):
            self.invalidate_struct()
        if new_graph.num_node > self.n_nodes:
            self._grow(new_graph.num_node, nfeats, None, new_graph)  # (swaps the graph in with the tables)
        else:
            self.graph = new_graph
        if torch.is_tensor(new_graph.last_batch[0]):  # extended on the device: the batch is already there
            src, dst, ts, eids = new_graph.last_batch
        return self.stream_step(src, dst, dst if neg is None else neg, ts, eids, want_prev=want_prev)

    @torch.no_grad()
    def observe_late(self, src, dst, ts, eids, *, efeats=None, num_node=None, nfeats=None):
        """Admit LATE events: a batch in any order whose times may lie before, inside or after what the model has seen (a
        client that was offline, a slow partition of a message bus, a settlement booked hours after the fact) -> the new
        graph.  Their edge-feature rows (efeats [n, d_e], for a model with an edge table) are appended to the table and
        the graph is replaced by `graph.merged(...)` through the setter (the restarter follows, snapshot stamps go stale,
        a prefetched collate part is dropped as for `forget`): every event stands in the rows of its two endpoints at the
        place its time gives it.  num_node / nfeats: as in `observe` - new node ids are admitted with the batch, the
        per-node tables grow (`grow_nodes`).  NOTHING IS STREAMED: both memories and the mailbox are not touched.
        THE LIMITS:
          * A late event changes what is READ from the graph from now on: sampled neighbours, the sequence restarter's
            histories, `exclude_seen`, `walk_candidates`, `trending`, `fill_candidates`.
          * It cannot be replayed into the recurrent state of its endpoints: that state has already consumed later
            events, and a GRU cannot be rewound.  Memories and pending mail are what they were.
          * Batches streamed before the call did not see the event - their embeddings and the state they left are not
            recomputed.
          * The caller's duties are those of `forget`: captured device graphs and resident evaluation runs built before
            the call read the old graph (and, after growth, the old tables) - rebuild them; CatalogueSnapshots held from
            before are stale.
        Refused before anything changes: a partitioned model, training mode, a stream capture in progress when tables
        would grow, efeats of another shape, and what `Graph.merged` refuses (a NaN time, ids outside [0, num_node), an
        eid that is no row of the edge table after the append, arrays of unequal length).  `observe` keeps refusing a
        batch that starts before the latest event: the two do not overlap."""
        self._refuse_partitioned('observe_late')
        self._refuse_tracked('observe_late')
        if self.training:
            raise RuntimeError('observe_late: late events are admitted in eval() mode (the streaming state of a served model)')
        if num_node is None and nfeats is not None:
            raise ValueError('observe_late: nfeats are the feature rows of newly admitted node ids (pass num_node)')
        fg = self.raw_feat_getter
        n = len(src)
        if efeats is not None and fg.efeats is not None:
            efeats = torch.as_tensor(efeats)
            if efeats.dim() != 2 or efeats.shape[0] != n or efeats.shape[1] != fg.efeats.shape[1]:
                raise ValueError(f'observe_late: efeats {tuple(efeats.shape)} for {n} events of width {fg.efeats.shape[1]}')
        grows = efeats is not None and fg.efeats is not None and n > 0
        if grows and self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('observe_late: tables cannot grow while a stream is being captured into a graph')
        rows = None if fg.efeats is None else fg.efeats.shape[0] + (n if efeats is not None else 0)
        # (validates, the eids against the table's rows included, before any launch; nothing has changed if it raises)
        if num_node is None:
            new_graph = self.graph.merged(src, dst, ts, eids, eid_rows=rows)
        else:
            new_graph = self.graph.merged(src, dst, ts, eids, eid_rows=rows, num_node=num_node)
            nfeats = self._grow_refusals('observe_late', max(new_graph.num_node, self.n_nodes), nfeats, None)
        if efeats is not None and fg.efeats is not None and fg.append_edge_rows(efeats):
            self.invalidate_struct()
        if new_graph.num_node > self.n_nodes:
            self._grow(new_graph.num_node, nfeats, None, new_graph)  # (swaps the graph in with the tables)
        else:
            self.graph = new_graph
        return self.graph

    def observe_late_keys(self, idmap, src_keys, dst_keys, ts, eids, *, efeats=None, nfeats=None):
        """`observe_late` for a stream that names its nodes by external int64 keys: the batch's keys are assigned dense ids
        by `idmap` in EVENT order, exactly as `observe_keys` assigns them (a key the map does not hold gets the next id, or
        a recycled one; nfeats may be a callable handed the admitted keys), and the batch is merged with num_node =
        max(idmap.size, n_nodes) -> the new graph.  Refusals and their order are those of `observe_keys`: what
        `observe_late` refuses about the batch is refused AFTER the assignment - the model is untouched, the keys stay."""
        self._refuse_tracked('observe_late_keys')
        src_keys = self._device_keys('observe_late_keys', 'src_keys', src_keys).reshape(-1)
        dst_keys = self._device_keys('observe_late_keys', 'dst_keys', dst_keys).reshape(-1)
        if src_keys.numel() != dst_keys.numel():
            raise ValueError('observe_late_keys: src_keys and dst_keys must have one entry per event')
        keys = torch.stack([src_keys, dst_keys], 1).reshape(-1)  # event order
        self._keyed_refusals('observe_late_keys', idmap, keys)
        if idmap.n_free == 0:
            ids = idmap.assign(keys).view(-1, 2).long()
            num_node = max(idmap.size, self.n_nodes)
            if callable(nfeats):
                nfeats = nfeats(idmap.key_of[self.n_nodes:num_node])
        else:
            ids, num_node = self._admit_recycled('observe_late_keys', idmap, keys, nfeats)
            ids, nfeats = ids.view(-1, 2).long(), None
        return self.observe_late(ids[:, 0].contiguous(), ids[:, 1].contiguous(), torch.as_tensor(ts).to(self.device),
                                 torch.as_tensor(eids).to(self.device), efeats=efeats, num_node=num_node, nfeats=nfeats)

    def _grow_refusals(self, what: str, num_node, nfeats, reserve):
        """everything grow_nodes refuses, before anything has changed -> the feature rows of the new ids (a tensor, or the
        count of zero rows)"""
        self._refuse_partitioned(what)
        if self.training:
            raise RuntimeError(f'{what}: node ids are admitted in eval() mode (the streaming state of a served model)')
        num_node = operator.index(num_node)
        k = num_node - self.n_nodes
        if k < 0:
            raise ValueError(f'{what}: num_node = {num_node} is below the model\'s {self.n_nodes} (node ids are never released)')
        if num_node > 0x7FFFFFFF:
            raise ValueError(f'{what}: node ids must fit in 31 bits')
        from .restarters import StaticRestarter
        if k and isinstance(getattr(self, 'restarter_fn', None), StaticRestarter):
            raise NotImplementedError(f'{what}: the static restarter holds one TRAINED embedding row per node; a new node has '
                                      'none, and resizing a parameter under an optimizer is not supported')
        if k and self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{what}: tables cannot grow while a stream is being captured into a graph')
        fg = self.raw_feat_getter
        if k and fg.nfeats is None:
            raise NotImplementedError(f'{what}: the feature getter has no node table (n_nodes is its row count)')
        if k and not fg.pin_mem:
            raise NotImplementedError(f'{what}: the node table lives in pinned host memory (register_buffer=False)')
        if k and not (fg.nfeats.shape[0] == self.left_memory.n == self.right_memory.n == self.msg_store.n == self.n_nodes):
            raise RuntimeError(f'{what}: the per-node tables do not all hold n_nodes = {self.n_nodes} rows')
        if self.graph.num_node > num_node:
            raise ValueError(f'{what}: the graph covers {self.graph.num_node} node ids, more than num_node = {num_node}')
        if reserve is not None and int(reserve) < num_node:
            raise ValueError(f'{what}: reserve = {reserve} rows is below num_node = {num_node}')
        if nfeats is not None:
            nfeats = torch.as_tensor(nfeats)
            if nfeats.dim() != 2 or nfeats.shape[0] != k or (k and nfeats.shape[1] != fg.nfeats.shape[1]):
                raise ValueError(f'{what}: nfeats {tuple(nfeats.shape)} for {k} new node ids of width {self.nfeat_dim}')
        if k:  # the step buffers are about to be dropped: a deferred invariant word of an earlier batch is read first
            self._poll_train_errors()
        return k if nfeats is None else nfeats

    def _grow(self, num_node: int, nfeats, reserve, graph) -> bool:
        """grow_nodes after its refusals: tables, counts, graph, caches"""
        eager, n0 = self._pending is not None, int(self.n_nodes)
        moved = [self.left_memory.grow(num_node, reserve), self.right_memory.grow(num_node, reserve),
                 self.msg_store.grow(num_node, reserve), self.raw_feat_getter.append_node_rows(nfeats, reserve)]
        self.n_nodes = num_node
        if getattr(self, 'restarter_fn', None) is not None:
            self.restarter_fn.n_nodes = num_node
        if self._tracker is not None:
            self._tracker.fit(num_node)  # (the admitted ids are born with zero rows: a snapshot cannot have read them)
        if self._journal is not None:  # (rows a delta's own growth does not rebuild: the feature rows the ids came with)
            self._journal.admitted(n0 if torch.is_tensor(nfeats) else num_node, num_node)
        self.graph = graph  # (the setter: the restarter follows)
        self._touch()
        self.invalidate_struct()
        # whatever was sized by the old count: step buffers (bitmaps, caps, the prefetched collate part), per-node tables
        self._step_ws = {k: v for k, v in self._step_ws.items() if k == 'rng'}
        self._gtab = self._ctab = self._gtab_stamp = None
        self._pending = self._pending_stamp = None
        if eager:
            self.eager_updates()  # a zeroed table of the new size: rebuilt from the state before the next eager step
        return any(moved)

    def grow_nodes(self, num_node: int, nfeats=None, reserve: Optional[int] = None) -> bool:
        """Admit the node ids [n_nodes, num_node) online -> whether a table's data pointer moved.  The two memories, the
        mailbox and the node-feature table get rows for them - zero state and no message, exactly the rows of a freshly
        built model; nfeats [num_node - n_nodes, d_n] are their feature rows (zeros if omitted) -, n_nodes changes on the
        model, the restarter and the feature getter, and the graph is replaced by `graph.widened(num_node)` if it is
        narrower.  From then on the model is, bit for bit, the model that was built on num_node nodes: `observe` /
        `stream_step` / `recommend` accept the new ids, and a checkpoint taken now loads into such a model.  Every table
        is the leading view of a backing store that grows by half (reserve=: rows of the new stores - memories, mailbox
        and node table alike -, for a caller that knows how far the ids will go), so most calls copy nothing and move no pointer; the stores are born zeroed and
        no kernel writes a row at or beyond n_nodes (each bounds its ids by the n_nodes of the struct it is handed).
        Dropped, because they were sized by the old count: the step buffers of `step_buffers` (their bitmaps, caps and
        prefetched batch), the eager-update and query tables (rebuilt before the next eager step).
        WHAT THE CALLER MUST DO AFTERWARDS (as after `release_edge_rows`): captured device graphs and resident evaluation
        runs built before a growth read the old tables and the old count - rebuild them; `uptodate` bitmaps go through
        `hip_ops.bitmap_grown`; StepBuffers and CatalogueSnapshots held from before are stale; a `save_memory_state` from
        before holds fewer rows and is refused by `load_memory_state` until its three modules were grown (`grow(n)`).
        Refused before anything runs - nothing has changed if it raises: a partitioned model, training mode, a model
        with a StaticRestarter (its per-node embeddings are trained parameters), growth while a stream is being captured,
        a model without a node-feature table or with one in pinned host memory, num_node below n_nodes or the graph's
        count or above 2^31 - 1, nfeats of another shape, reserve below num_node."""
        nfeats = self._grow_refusals('grow_nodes', num_node, nfeats, reserve)
        num_node = operator.index(num_node)
        if num_node == self.n_nodes:
            return False
        graph = self.graph if self.graph.num_node == num_node else self.graph.widened(num_node)
        return self._grow(num_node, nfeats, reserve, graph)

    # ---- compacting the node id space ------------------------------------------------------------------------
    def _compact_refusals(self, what: str):
        """everything a compaction refuses that can be told before the plan, with nothing changed"""
        self._refuse_partitioned(what)
        if self.training:
            raise RuntimeError(f'{what}: node ids are compacted in eval() mode (the streaming state of a served model)')
        from .restarters import StaticRestarter
        if isinstance(getattr(self, 'restarter_fn', None), StaticRestarter):
            raise NotImplementedError(f'{what}: the static restarter holds one TRAINED embedding row per node; resizing a '
                                      'parameter under an optimizer is not supported')
        if self.device.type != 'cuda':
            raise RuntimeError(f'{what}: the model lives on {self.device}; node ids are compacted on the GPU')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{what}: tables cannot be compacted while a stream is being captured into a graph')
        fg = self.raw_feat_getter
        if fg.nfeats is None:
            raise NotImplementedError(f'{what}: the feature getter has no node table (n_nodes is its row count)')
        if not fg.pin_mem:
            raise NotImplementedError(f'{what}: the node table lives in pinned host memory (register_buffer=False)')
        if not (fg.nfeats.shape[0] == self.left_memory.n == self.right_memory.n == self.msg_store.n == self.n_nodes):
            raise RuntimeError(f'{what}: the per-node tables do not all hold n_nodes = {self.n_nodes} rows')
        if self.graph.num_node > self.n_nodes:
            raise RuntimeError(f'{what}: the graph covers {self.graph.num_node} node ids, more than n_nodes = {self.n_nodes}')

    def _compact_plan(self, what: str, drop_bits: Tensor, n_ids: int):
        """-> (the plan, the graph it was made over: the model's, widened to n_nodes if it covers fewer ids); the ROW / NBR
        classes name the id and say what to do"""
        g = self.graph if self.graph.num_node == self.n_nodes else self.graph.widened(self.n_nodes)
        g.tcsr  # (a graph that was never sampled from has no device arrays yet)
        plan = hip_ops.node_compact_plan(g, drop_bits, n_ids, strict=False)
        if plan.code in (hip_ops._lib.TG_NODE_COMPACT_ROW, hip_ops._lib.TG_NODE_COMPACT_NBR):
            node = plan.first if plan.code == hip_ops._lib.TG_NODE_COMPACT_ROW else int(g._dev[2][plan.first])
            how = 'still owns entries of the graph' if plan.code == hip_ops._lib.TG_NODE_COMPACT_ROW else \
                f'is still the neighbour of entry {plan.first} of the graph'
            raise ValueError(f'{what}: node {node} is dropped but {how}: `erase` it first '
                             f'({hip_ops.NODE_COMPACT_CLASSES[plan.code - 1]})')
        if plan.code:
            raise ValueError(f'{what}: ' + hip_ops.NODE_COMPACT_TEXT(plan.code, plan.first, n_ids))
        return plan, g

    def _compact(self, plan, graph, reserve):
        """a compaction after its refusals: everything is BUILT first - child graph, new tables -, then swapped in one step"""
        from .memory import compact_tables
        self._poll_train_errors()  # (the step buffers are about to be dropped: a deferred invariant word is read first)
        n_new = plan.n_graph_new
        old_of = plan.old_of[:n_new]  # (monotone: the kept ids below n_nodes are a prefix)
        L, R, S, fg = self.left_memory, self.right_memory, self.msg_store, self.raw_feat_getter
        child = graph.compacted(plan)
        built = compact_tables([(m, name) for m in (L, R, S) for name in m.COMPACT_TABLES], old_of, reserve)  # 8 tables, ONE launch
        bits = S._compacted_bits(old_of, built[0][2].shape[0])
        node_rows = fg._compact_build(old_of, reserve)
        # ---- nothing has changed up to here; nothing below can raise ----
        eager = self._pending is not None
        L._adopt_compacted(built[0:3])
        R._adopt_compacted(built[3:6])
        S._adopt_compacted(built[6:8], bits)
        fg._adopt_compacted(node_rows)
        self.n_nodes = n_new
        if getattr(self, 'restarter_fn', None) is not None:
            self.restarter_fn.n_nodes = n_new
        for sink in self._sinks():  # another numbering: a bitmap over the old ids means nothing any more
            sink.renumbered(n_new)  # (the tracker: a new epoch, no snapshot from before is refreshable)
        self.graph = child  # (the setter: the restarter follows; snapshot stamps go stale)
        self._touch()
        self.invalidate_struct()
        self._step_ws = {k: v for k, v in self._step_ws.items() if k == 'rng'}
        self._gtab = self._ctab = self._gtab_stamp = None
        self._pending = self._pending_stamp = None
        if eager:
            self.eager_updates()

    @torch.no_grad()
    def compact_nodes(self, drop, reserve: Optional[int] = None, *, bitmap: bool = False):
        """Take erased node ids OUT of the id space: the remaining ids are renumbered densely IN THEIR ORDER and everything
        sized by n_nodes shrinks - both memories, the mailbox, the node table, the graph's indptr (tg_node_compact.hip;
        DESIGN 7.20) -> the NodeCompaction (remap, old_of, n_old, n_new, translate, bitmap).  drop: int64 node ids
        (a sequence or tensor; duplicates are fine) or, with bitmap=True, a bitmap over n_nodes ids (`hip_ops.new_bitmap`
        words on the model's device, a set bit = the id leaves).  A dropped id must have been erased (`erase`): it owns no entry and is
        nobody's neighbour.  Because the remap is monotone every "ascending id" / "ascending column" tie-break survives:
        the compacted model is the uncompacted one under `remap`, bit for bit, for every product.
        Everything is built first - plan (ONE read-back), child graph (`Graph.compacted`: ts / eid shared with the
        parent), new tables (new zeroed backing stores with the head-room of `grow_capacity`, reserve=: their rows; the
        eight tables of memories and mailbox move in ONE launch) - and then swapped in one step: if anything raises,
        nothing has changed.  Peak memory is old table + new table (no in-place compaction).  Then, as `grow_nodes`:
        n_nodes changes on the model, the restarter and the feature getter, the graph goes through the setter, step
        buffers (but the dropout generator) and the eager-update and query tables are dropped and rebuilt before their
        next use.  An empty `drop` returns the identity plan and changes nothing.
        WHAT THE CALLER MUST DO AFTERWARDS: captured device graphs and resident evaluation runs are rebuilt; `uptodate`
        bitmaps go through `plan.bitmap`; node ids it holds go through `plan.translate` (-1: dropped); StepBuffers and
        CatalogueSnapshots from before are stale - a snapshot of the old numbering is REFUSED by `recommend` through its
        stamp, never remapped; a `save_memory_state` from before no longer fits.
        Refused before anything changes: a partitioned model, training mode, a model with a StaticRestarter (its rows are
        trained parameters under an optimiser), a stream capture in progress, a node table in pinned host memory or no
        node table, per-node tables (or a graph) that do not all hold n_nodes rows, id 0 or an id outside [0, n_nodes),
        and a dropped id that still owns entries or is still a neighbour (the id is named: `erase` it first)."""
        self._compact_refusals('compact_nodes')
        n = self.n_nodes
        if bitmap:
            if not (torch.is_tensor(drop) and drop.dtype == torch.int64 and drop.dim() == 1 and drop.is_contiguous()
                    and drop.device == self.device and drop.numel() >= hip_ops.bitmap_words(n)):
                raise ValueError(f'compact_nodes: a bitmap over {n} ids is a contiguous int64 tensor of '
                                 f'{hip_ops.bitmap_words(n)} words on {self.device}')
            bits = drop
        else:
            ids = torch.as_tensor(drop)
            if ids.numel() and (ids.dtype.is_floating_point or ids.dtype == torch.bool):
                raise ValueError(f'compact_nodes: drop holds integer node ids (bitmap=True: a bitmap), not {ids.dtype}')
            ids = ids.to(self.device, torch.int64).reshape(-1)
            if ids.numel():
                lo, hi = (int(x) for x in torch.aminmax(ids))
                if lo < 0 or hi >= n:
                    raise ValueError(f'compact_nodes: node ids must lie in [0, n_nodes) (n_nodes = {n})')
                if lo == 0:
                    raise ValueError('compact_nodes: node id 0 is the padding id and can never be dropped')
            bits = hip_ops.new_bitmap(n, self.device)
            if ids.numel():
                hip_ops.bitmap_mark(ids, bits, n)
        plan, graph = self._compact_plan('compact_nodes', bits, n)
        if not plan.identity:
            self._compact(plan, graph, reserve)
        return plan

    @torch.no_grad()
    def compact_keys(self, idmap, reserve: Optional[int] = None):
        """`compact_nodes` behind an id map: the ids the map holds FREE (after `erase_keys`) leave the model AND the map ->
        the NodeCompaction.  ONE plan over max(idmap.size, n_nodes) ids with drop_bits = idmap.free_bits serves both sides.
        Ids in [n_nodes, idmap.size) are assigned but never admitted (the batch that brought their key was refused): they
        have no model rows and are kept or dropped like any other; the model's new n_nodes is the number of kept ids below
        the old one, the map's new size the number below its old size.  The model side is validated and built before the
        map is touched, and the map builds its new tables before it swaps them: if the call raises, neither has changed.
        Afterwards idmap.size = live keys + 1, n_free = 0, its capacity has SHRUNK to what the live keys need, and
        `observe_keys` / `recommend_keys` go on as before.  Nothing free: the identity plan, nothing changes.  The caller's
        duties and the refusals are those of `compact_nodes`; also refused: a map on another device, a map that holds
        fewer ids than the model has admitted."""
        self._compact_refusals('compact_keys')
        if idmap.device != self.device:
            raise ValueError(f'compact_keys: the id map lives on {idmap.device}, the model on {self.device}')
        if idmap.size < self.n_nodes:
            raise ValueError(f'compact_keys: the id map holds {idmap.size} ids, the model has admitted {self.n_nodes}')
        plan, graph = self._compact_plan('compact_keys', idmap.free_bits, idmap.size)
        if plan.identity:
            return plan
        # the map's side is checked before the model changes (IdMap.compact repeats it)
        if plan.rows_below(idmap.size) != idmap.size - idmap.n_free:
            raise ValueError(f'compact_keys: the map\'s bitmap holds {idmap.size - plan.n_new} free ids, the map counts '
                             f'{idmap.n_free}')
        built_map = idmap._compact_build(plan)
        self._compact(plan, graph, reserve)
        idmap._compact_adopt(built_map)
        return plan

    # ---- serving behind external keys (data/idmap.py: IdMap) ------------------------------------------------
    def _device_keys(self, what: str, name: str, keys) -> Tensor:
        keys = torch.as_tensor(keys)
        if keys.dtype != torch.int64:
            raise ValueError(f'{what}: {name} are int64 keys, not {keys.dtype}')
        return keys.to(self.device).contiguous()

    def _keyed_refusals(self, what: str, idmap, keys: Tensor):
        """what an admission of the keys' new ids would be refused for and that can be told WITHOUT the ids - before a key
        is assigned"""
        self._refuse_partitioned(what)
        if self.training:
            raise RuntimeError(f'{what}: keys are admitted in eval() mode (the streaming state of a served model)')
        if idmap.device != self.device:
            raise ValueError(f'{what}: the id map lives on {idmap.device}, the model on {self.device}')
        if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{what}: assigning keys reads the new size back; it cannot be captured into a graph')
        from .restarters import StaticRestarter
        if isinstance(getattr(self, 'restarter_fn', None), StaticRestarter):
            unknown = int((idmap.lookup(keys) < 0).sum()) if keys.numel() else 0
            if unknown or idmap.size > self.n_nodes:
                raise NotImplementedError(f'{what}: {unknown} keys are new, and the static restarter holds one TRAINED '
                                          'embedding row per node; a new node has none')

    def observe_keys(self, idmap, src_keys, dst_keys, ts, eids, **observe_kwargs):
        """`observe` for a stream that names its nodes by external int64 keys: the batch's keys are assigned dense ids by
        `idmap` (an IdMap on the model's device) in EVENT order - src[0], dst[0], src[1], dst[1], ... - and the batch is
        observed with num_node = max(idmap.size, n_nodes) -> the step's StepBuffers.  A key the map does not hold gets
        the next id in the order of first appearance, so a stream gets the same ids - and the model ends in the same
        state, bit for bit - however it is cut into batches, and a model built on dense ids goes behind keys with
        `IdMap.from_keys` without being renumbered.  One read-back (the new size) on top of observe's.
        observe_kwargs: those of observe but num_node.  nfeats may be a CALLABLE: it is handed the keys (int64, device) of
        the ids the model is about to admit, [n_nodes, idmap.size), and returns their feature rows.
        A map that holds FREE ids (after `erase_keys`) hands them out first: the ids to admit are then the recycled ids
        below n_nodes given out by this call, in assignment order, followed by [n_nodes, idmap.size); nfeats holds one row
        for each of them in that order (a callable is handed their keys).  The model grows with zero rows to idmap.size and
        the rows are written in place (`set_node_rows`) BEFORE observe: if observe then refuses the batch, the keys stay
        assigned, as without free ids, and so do their feature rows and the zero rows the growth added; what memories,
        mailbox and graph held is untouched.
        Refused before a key is assigned: a partitioned model, training mode, a captured stream, a map on another
        device, keys that are no int64, and - with a static restarter - a batch that holds a key the map does not.
        Whatever else observe / grow_nodes refuse (a batch that goes back in time, an eid that is no row, feature rows of
        another shape, ...) is refused AFTER the assignment: the model is untouched, but the keys stay assigned - a key
        may precede its first event; the next observe_keys admits its id with the batch it arrives in."""
        if 'num_node' in observe_kwargs:
            raise TypeError('observe_keys: num_node follows from the id map')
        self._refuse_tracked('observe_keys')
        src_keys = self._device_keys('observe_keys', 'src_keys', src_keys).reshape(-1)
        dst_keys = self._device_keys('observe_keys', 'dst_keys', dst_keys).reshape(-1)
        if src_keys.numel() != dst_keys.numel():
            raise ValueError('observe_keys: src_keys and dst_keys must have one entry per event')
        keys = torch.stack([src_keys, dst_keys], 1).reshape(-1)  # event order
        self._keyed_refusals('observe_keys', idmap, keys)
        nfeats = observe_kwargs.pop('nfeats', None)
        if idmap.n_free == 0:
            ids = idmap.assign(keys).view(-1, 2).long()
            num_node = max(idmap.size, self.n_nodes)
            if callable(nfeats):
                nfeats = nfeats(idmap.key_of[self.n_nodes:num_node])
        else:
            ids, num_node = self._admit_recycled('observe_keys', idmap, keys, nfeats)
            ids, nfeats = ids.view(-1, 2).long(), None
        return self.observe(ids[:, 0].contiguous(), ids[:, 1].contiguous(), torch.as_tensor(ts).to(self.device),
                            torch.as_tensor(eids).to(self.device), num_node=num_node, nfeats=nfeats, **observe_kwargs)

    def _admit_recycled(self, what: str, idmap, keys: Tensor, nfeats):
        """assign `keys` on a map that holds free ids and admit what the call gave out -> (ids int32 [n], num_node): the
        recycled ids below n_nodes in assignment order, then [n_nodes, idmap.size).  nfeats (a tensor, a callable handed
        the keys of those ids, or None for zero rows) is checked first; then the model grows with zero rows and the rows
        are written in place (set_node_rows) - a recycled id's row is overwritten, not appended."""
        n0 = self.n_nodes
        ids, new_ids = idmap.assign(keys, return_new=True)
        num_node = max(idmap.size, n0)
        admit = torch.cat([new_ids[new_ids < n0].long(), torch.arange(n0, num_node, device=self.device)])
        if callable(nfeats):
            nfeats = nfeats(idmap.key_of[admit])
        if nfeats is not None:
            nfeats = torch.as_tensor(nfeats)
            if nfeats.dim() != 2 or nfeats.shape[0] != admit.numel() or nfeats.shape[1] != self.nfeat_dim:
                raise ValueError(f'{what}: nfeats {tuple(nfeats.shape)} for {admit.numel()} admitted node ids of width '
                                 f'{self.nfeat_dim}')
        if num_node > n0:
            self.grow_nodes(num_node)
        if admit.numel() and self.raw_feat_getter.nfeats is not None:
            self.set_node_rows(admit, 0 if nfeats is None else nfeats, check=False)
        return ids, num_node

    def set_node_rows(self, ids, rows, check: bool = True):
        """`NumericalFeature.set_node_rows(ids, rows)` on the model's node table, and the tables derived from it (eager
        updates, centre / query rows) are rebuilt before their next use.  Its refusals."""
        self.raw_feat_getter.set_node_rows(ids, rows, check=check)
        self._touch()
        self._mark(ids)

    def erase_keys(self, idmap, keys, *, eids=None, release_edge_rows: bool = False, keep_from=None):
        """`erase` behind external keys, and the keys LEAVE the map (a closed account) -> (graph,
        removed_ids): the new graph and the dense ids the map released, int32, ascending.  In this order:
          1. the keys are looked up; a key the map does not hold is ignored, and so is INT64_MIN;
          2. `erase(nodes = the ids the model has admitted, eids=eids, release_edge_rows=, keep_from=)` - it validates
             everything, and nothing has changed if it raises;
          3. the node-feature rows of the erased ids are zeroed (`set_node_rows(ids, 0)`): with step 2 every per-node row
             is that of a freshly built model;
          4. `idmap.remove(keys)`: the ids are free and are handed out again, the smallest first, by the next
             `observe_keys` / `recommend_keys(admit=True)` - n_nodes stays at the peak of live keys (+ the free ones).
        A key that was assigned but not yet admitted (its id is >= n_nodes: the batch that brought it was refused) is only
        removed from the map.  A key that comes back later is a new key: a node never seen, possibly under another id.
        `erase`'s LIMITS carry over unchanged: partners' memories and pending mail keep what the node contributed, and a
        recycled id inherits nothing but that - no row of its own.  THE CALLER'S DUTIES are those of `erase`, and for
        `uptodate` bitmaps held from lazy restarts: clear the bits of removed_ids (a recycled id is a node never seen).
        Refused before anything changes: what `_keyed_refusals` refuses (a partitioned model, training mode, a map on
        another device, a captured stream, a static restarter with unknown keys), keys that are no int64, a node table in
        pinned host memory, and what `erase` refuses."""
        keys = self._device_keys('erase_keys', 'keys', keys).reshape(-1)
        self._keyed_refusals('erase_keys', idmap, keys)
        fg = self.raw_feat_getter
        if fg.nfeats is not None and not fg.pin_mem:
            raise NotImplementedError('erase_keys: the node table lives in pinned host memory (register_buffer=False)')
        ids = idmap.lookup(keys).long()
        nodes = ids[(ids > 0) & (ids < self.n_nodes)]
        graph = self.graph
        if nodes.numel() or eids is not None:
            graph = self.erase(nodes=nodes if nodes.numel() else None, eids=eids, release_edge_rows=release_edge_rows,
                               keep_from=keep_from)
        if nodes.numel() and fg.nfeats is not None:
            self.set_node_rows(nodes, 0, check=False)   # (a fill: duplicates are fine)
        _, removed = idmap.remove(keys)
        return graph, removed

    def recommend_keys(self, idmap, src_keys, ts, cand, k: int, *, cand_keys=None, admit: bool = False, **recommend_kwargs):
        """`recommend` behind external keys -> (keys int64 [B, k], scores float32 [B, k], n_valid int32 [B]); keys =
        idmap.keys_of(ids), so positions past n_valid[i] hold INT64_MIN, the key of the padding id.
        cand: a CatalogueSnapshot or a tensor of dense ids, as in recommend - or None with cand_keys=, a tensor of keys
        ([C] or [B, C]) that is looked up: a candidate the map does not hold, or whose id the model has not admitted yet,
        becomes the padding id 0 and is thereby left out.
        The sources are looked up.  admit=False: a source the map (or the model) does not know raises ValueError saying
        how many - one read-back - and nothing has changed.  admit=True: unknown sources are ASSIGNED (in their order in
        src_keys) and the model grows to idmap.size (grow_nodes): a brand-new user is a zero-state node without history -
        `recommend_walk`'s fill= is what gives such a user a list worth showing.  What an admission is refused for is
        refused as in observe_keys."""
        if (cand is None) == (cand_keys is None):
            raise ValueError('recommend_keys: pass cand (a snapshot or dense ids) or cand_keys=, one of them')
        src_keys = self._device_keys('recommend_keys', 'src_keys', src_keys).reshape(-1)
        if idmap.device != self.device:
            raise ValueError(f'recommend_keys: the id map lives on {idmap.device}, the model on {self.device}')
        if cand_keys is not None:
            cand_keys = self._device_keys('recommend_keys', 'cand_keys', cand_keys)
        if admit:
            self._keyed_refusals('recommend_keys', idmap, src_keys)
            if idmap.n_free == 0:
                ids = idmap.assign(src_keys)
                if idmap.size > self.n_nodes:
                    self.grow_nodes(idmap.size)
            else:  # (ids that were released are handed out first: their rows are those of a node never seen)
                ids, _ = self._admit_recycled('recommend_keys', idmap, src_keys, None)
        else:
            ids = idmap.lookup(src_keys)
            unknown = int(((ids < 0) | (ids >= self.n_nodes)).sum())
            if unknown:
                raise ValueError(f'recommend_keys: {unknown} of the {ids.numel()} sources are keys the model has never seen '
                                 '(admit=True assigns them ids and grows the model)')
        if cand_keys is not None:  # (after an admission: the model's count is the one the candidates are held against)
            cand = idmap.lookup(cand_keys.reshape(-1)).long().view(cand_keys.shape)
            cand = torch.where((cand < 0) | (cand >= self.n_nodes), torch.zeros_like(cand), cand)
        out, scores, n_valid = self.recommend(ids.long(), ts, cand, k, **recommend_kwargs)
        return idmap.keys_of(out, check=False), scores, n_valid

    def forget(self, before=None, keep_last=None, release_edge_rows: bool = False, keep_from=None):
        """Sliding-window expiry for a model that keeps observing: the graph is replaced by `graph.trimmed(before,
        keep_last)` (entries with a time strictly below `before`, and entries that are not among their node's last
        `keep_last`, are dropped) -> the new graph.  Only the graph changes: memories, mailbox and tables are not touched,
        and by default the edge-feature table keeps its rows (eids are row indices).  A one-layer `recent_edges` model with
        n_neighbors and hist_len <= keep_last that forgets after every `observe` stays bit-identical to one that never
        forgets; a two-layer model does not (hop 2 is sampled at the neighbours' earlier times).  Afterwards
        `recommend(..., exclude_seen=True)` means "seen inside the window".
        release_edge_rows=True: the trim is followed by `release_edge_rows(keep_from)` - the rows that no kept entry names
        leave the table and the eids are renumbered; the result is `model.last_release` (None without an edge table) and
        the caller translates the eids it holds as that method says.  The model still computes what it would have.
        Refused before anything runs: a partitioned model, and what `Graph.trimmed` refuses (a NaN `before`, a negative
        `keep_last`); with the flag also what `release_edge_rows` refuses, and then nothing at all has changed."""
        self._refuse_partitioned('forget')
        return self._swap_graph(self.graph.trimmed(before=before, keep_last=keep_last), release_edge_rows, keep_from)

    def _swap_graph(self, child, release_edge_rows: bool, keep_from):
        """the tail of `forget` and `erase`: `child` becomes the graph, alone or together with the packed edge table"""
        if release_edge_rows:
            self.release_edge_rows(keep_from=keep_from, _graph=child)  # (swaps graph and table together, or raises)
        else:
            self.graph = child
        return self.graph

    @torch.no_grad()
    def erase(self, nodes=None, eids=None, *, release_edge_rows: bool = False, keep_from=None):
        """Take particular nodes and particular events out of a model that keeps observing (a closed account, a de-listed
        item, a cancelled or fraudulent transaction) -> the new graph.  The graph is replaced by `graph.without(nodes,
        eids, eid_rows=rows of the edge table)` through the setter (the restarter follows, snapshot stamps go stale):
        every entry whose owner or neighbour is one of `nodes`, or whose eid is one of `eids`, is gone, so
        `walk_candidates`, `trending`, `fill_candidates`, `exclude_seen`, the samplers and the sequence restarter's
        histories no longer see it.  For every id of `nodes` the rows of both memories (vals, update_ts, active_mask) and
        the mailbox row (values, time, has_msg bit) are put back to those of a freshly built model - zeros, no message -
        and nothing else is touched; derived tables (eager updates, query rows) are rebuilt before their next use.
        (`reset()` clears a mailbox row's bit and leaves its values behind it, where nothing reads them; an erase zeroes
        them too: the last message of a closed account does not stay in device memory.)
        nodes / eids: int sequences or tensors, duplicates are fine, an eid that names no entry is a no-op.
        release_edge_rows=True: the erase is followed by `release_edge_rows(keep_from)`, exactly as in `forget` - the rows
        that only retracted events named leave the table, the eids are renumbered, the result is `model.last_release`.
        THE LIMITS:
          * Rows of OTHER nodes are not touched.  What an erased node or a retracted event contributed to a partner's
            recurrent memory or to its pending mail cannot be separated out again and stays.
          * A StaticRestarter's trained per-node embedding is not reset.
          * The caller's duties are those of `forget` and `release_edge_rows`: captured device graphs and resident
            evaluation runs built before the call read the old graph (and table) - rebuild them; CatalogueSnapshots held
            from before are stale; eids held by the caller are in the old numbering after a release.
          * An erased id that a later `observe` brings back starts as a node never seen.
        Refused before anything changes: a partitioned model, training mode, and what `Graph.without` refuses (an id
        outside [0, num_node), node id 0 - the padding id -, a negative eid, both arguments None); with the flag also
        what `release_edge_rows` refuses, and then nothing at all has changed."""
        self._refuse_partitioned('erase')
        if self.training:
            raise RuntimeError('erase: nodes and events are taken out in eval() mode (the streaming state of a served model)')
        fg = self.raw_feat_getter
        rows = None if eids is None or fg.efeats is None else int(fg.efeats.shape[0])
        child = self.graph.without(nodes, eids, eid_rows=rows)  # (validates; nothing has changed if it raises)
        ids = None
        if nodes is not None:
            ids = torch.as_tensor(nodes).to(self.device).long().reshape(-1)
        self._swap_graph(child, release_edge_rows, keep_from)
        if ids is not None and ids.numel():
            self.left_memory.clear(ids)
            self.right_memory.clear(ids)
            S = self.msg_store
            S.node_msg_vals.index_fill_(0, ids, 0)
            S.node_msg_ts.index_fill_(0, ids, 0)
            S.clear(ids)
            self._mark(ids)
        self._touch()
        return self.graph

    last_release = None  # the EdgeRowsRelease of the latest release_edge_rows / forget(release_edge_rows=True)

    def release_edge_rows(self, keep_from=None, pin=None, *, slack=None, _graph=None):
        """Release the edge-table rows of forgotten events: every row that no entry of the graph names any more leaves the
        table, the remaining rows are packed in their old order into a new table and the graph's eids are renumbered to
        match (NumericalFeature.compact_edge_rows, Graph.renumbered; tg_edge_rows.hip) -> EdgeRowsRelease(remap,
        rows_before, rows, shift), also kept as `model.last_release`; None (and nothing changes) for a model without an
        edge table.  Kept besides the rows the graph names: row 0 (padding), rows >= keep_from (default: none) - the rows
        the caller appended for events it has NOT observed yet -, and the ids of `pin`.  Afterwards the model computes,
        bit for bit, what it would have computed without the call: mailbox, memories, query tables and snapshots hold edge
        ROWS or no edge data at all, never an eid.
        Order: plan, one int64 read back (the only synchronisation), allocate, apply; only then graph (through the
        setter: the restarter follows), table and `invalidate_struct()`.  If anything raises, nothing has changed.  Peak
        memory is old table + new table.  The new table has head-room for the next `observe` (slack=: spare rows).
        WHAT THE CALLER MUST DO AFTERWARDS - eids it holds are in the old numbering:
          * pending events, a resident InteractionData: eid -> remap[eid], or eid - shift for ids >= keep_from;
          * the `l1_eids` of a step returned earlier are old numbers;
          * captured device graphs and resident evaluation runs built before the call read the old graph and the old
            table: rebuild them.
        Refused before anything runs: a partitioned model, a table in pinned host memory (register_buffer=False), a
        keep_from outside [0, rows], an entry or pin that names no row (ValueError)."""
        self._refuse_partitioned('release_edge_rows')
        fg = self.raw_feat_getter
        graph = self.graph if _graph is None else _graph
        res = fg.compact_edge_rows(graph, keep_from, pin, slack=slack, swap=False)
        if res is None:
            if _graph is not None:
                self.graph = _graph
            self.last_release = None
            return None
        child = graph.renumbered(res.remap, res.eid_out)
        # (an attached event-key tracker follows the rows: built beside the old one - it may raise -, swapped with the rest)
        events = None if self.events is None else self.events._released_build(res)
        self.graph = child
        if self._journal is not None:  # (a trim or an erase in the same call hides the shared indptr from the setter)
            self._journal.mark_all('release_edge_rows packed the edge table and renumbered every edge id')
        fg.adopt_edge_rows(res)
        if events is not None:
            self.events._adopt(events)
        self.invalidate_struct()
        self.last_release = res
        return res

    # ---- event keys: idempotent ingestion and retraction by external event id (data/events.py) -------------
    def _events_refusals(self, what: str):
        self._refuse_partitioned(what)
        fg = self.raw_feat_getter
        if fg.efeats is None:
            raise NotImplementedError(f'{what}: the model has no edge table; event keys name its rows (NOT BUILT for models '
                                      'without one)')
        if not fg.pin_mem:
            raise NotImplementedError(f'{what}: the edge table lives in pinned host memory (register_buffer=False)')
        if self.training:
            raise RuntimeError(f'{what}: events are tracked in eval() mode (the streaming state of a served model)')
        if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{what}: building the key table reads an error word back; it cannot be captured into a graph')

    def track_events(self, keys=None):
        """Name events by external int64 keys from now on -> the EventKeys tracker, also kept as `model.events`
        (data/events.py).  keys int64 [rows - 1]: the keys of the rows the edge table holds now (row 0 is the padding row);
        None: those rows are keyless - never matched, never retractable by key.  While the tracker is attached:
          * `observe_events` is idempotent and `retract_events` takes keys;
          * `release_edge_rows`, and the release paths of `forget` / `erase`, carry the tracker along inside the same
            all-or-nothing swap as graph and table (EventKeys.released);
          * plain `observe` / `observe_keys` / `observe_late*`, `load_online` and `apply_online_delta` raise RuntimeError:
            they would add or replace rows behind the tracker's back (detach, load, `attach_events` the restored tracker);
          * `compact_nodes` is unaffected (it renumbers nodes, not rows).
        THE LIMITS: the dedupe and tombstone horizon is the life of the edge row - after `forget(...,
        release_edge_rows=True)` a very old redelivery is unknown again (`observe_events` then refuses it as going back in
        time; late=True admits it).  The journal's deltas do not carry event keys: `events.state_dict()` is saved whole
        (8 B per row) beside `online_state()`, as an IdMap is; a delta form is NOT BUILT.  Models without an edge table
        are not supported.
        Refused before anything changes: a model without an edge table (NotImplementedError), a table in pinned host
        memory, a partitioned model, training mode, a stream capture in progress, and keys EventKeys refuses (another
        count than rows - 1, a key that stands twice, INT64_MIN)."""
        from ..data.events import EventKeys
        self._events_refusals('track_events')
        self.events = EventKeys(self.device, int(self.raw_feat_getter.efeats.shape[0]), keys)
        return self.events

    def attach_events(self, ev):
        """Attach a restored tracker (EventKeys.from_state_dict) -> it, also kept as `model.events`.  Refused before
        anything changes: what `track_events` refuses, a tracker whose size is not the edge table's row count, a tracker on
        another device (ValueError)."""
        self._events_refusals('attach_events')
        rows = int(self.raw_feat_getter.efeats.shape[0])
        if ev.size != rows:
            raise ValueError(f'attach_events: the tracker covers {ev.size} rows, the edge table has {rows}')
        if ev.device != self.device:
            raise ValueError(f'attach_events: the tracker lives on {ev.device}, the model on {self.device}')
        self.events = ev
        return ev

    def detach_events(self):
        """Remove the tracker -> it (or None): the model is fed by plain `observe` again"""
        ev, self.events = self.events, None
        return ev

    def observe_events(self, src, dst, ts, event_keys, *, efeats, idmap=None, late: bool = False, **observe_kwargs):
        """`observe` for a stream that names its EVENTS by external int64 keys and may deliver them more than once ->
        (step, EventAdmission(eids, keep, n_kept)).  In this order:
          1. `events.screen(event_keys)`: keep = the first occurrences of the keys never seen (the map is only read);
          2. src / dst / ts / efeats are gathered by keep;
          3. the kept events are observed with eids = rows + arange(n_kept): `observe`; with idmap= `observe_keys` (src / dst
             are then NODE keys - screened first, so a dropped duplicate assigns no node id); with late=True `observe_late`
             / `observe_late_keys` (the step is then the new graph);
          4. `events.commit(event_keys[keep])`.
        A redelivered event - a copy inside the batch, a copy of an earlier batch, a whole batch sent twice - changes
        nothing: the model ends bit-identical to one fed the clean stream through `observe`.  If step 3 raises, the tracker
        is unchanged (the screen wrote nothing; the table may have grown in capacity, the mapping has not).  n_kept == 0:
        nothing is observed and the step is None.  efeats [n, d_e] is required; the caller passes no eids.
        observe_kwargs: those of the call of step 3 (neg and nfeats are per-event / per-call as there; neg is gathered by
        keep).  THE LIMITS are those of `track_events`."""
        what = 'observe_events'
        ev = self.events
        if ev is None:
            raise RuntimeError(f'{what}: no event-key tracker is attached (track_events / attach_events)')
        if 'eids' in observe_kwargs:
            raise TypeError(f'{what}: eids follow from the tracker')
        fg = self.raw_feat_getter
        dev = self.device
        event_keys = self._device_keys(what, 'event_keys', event_keys).reshape(-1)
        n = event_keys.numel()
        efeats = torch.as_tensor(efeats).to(dev)
        if efeats.dim() != 2 or efeats.shape[0] != n or efeats.shape[1] != fg.efeats.shape[1]:
            raise ValueError(f'{what}: efeats {tuple(efeats.shape)} for {n} events of width {fg.efeats.shape[1]}')
        src, dst, ts = (torch.as_tensor(x).to(dev).reshape(-1) for x in (src, dst, ts))
        if not (src.numel() == dst.numel() == ts.numel() == n):
            raise ValueError(f'{what}: src, dst, ts and event_keys must have one entry per event')
        rows = int(fg.efeats.shape[0])
        if ev.size != rows:
            raise RuntimeError(f'{what}: the tracker covers {ev.size} rows, the edge table has {rows}: rows were added or '
                               'released behind its back')
        eids, keep = ev.screen(event_keys)
        m = int(keep.numel())
        if m == 0:
            return None, EventAdmission(eids, keep, 0)
        ev.reserve(m)   # (before the batch is observed: commit cannot fail for want of room)
        pick = lambda x: x.index_select(0, keep)
        if observe_kwargs.get('neg') is not None:
            observe_kwargs['neg'] = pick(torch.as_tensor(observe_kwargs['neg']).to(dev).reshape(-1))
        new_eids = torch.arange(rows, rows + m, dtype=torch.int64, device=dev)
        self._events_admitting = True
        try:
            if idmap is None:
                call = self.observe_late if late else self.observe
                step = call(pick(src), pick(dst), pick(ts), new_eids, efeats=pick(efeats), **observe_kwargs)
            else:
                call = self.observe_late_keys if late else self.observe_keys
                step = call(idmap, pick(src), pick(dst), pick(ts), new_eids, efeats=pick(efeats), **observe_kwargs)
        finally:
            self._events_admitting = False
        ev.commit(pick(event_keys))
        return step, EventAdmission(eids, keep, m)

    def retract_events(self, keys, *, release_edge_rows: bool = False, keep_from=None):
        """`erase(eids=...)` behind event keys (a chargeback names a transaction id) -> (graph, eids): the new graph and the
        rows (int64, in the order of `keys`) of the keys the tracker holds; a key it does not hold is ignored, and so is
        INT64_MIN.  Without a release the key STAYS mapped to its row, which no entry names any more: a redelivered copy of
        a retracted event stays dropped, like a tombstone.  release_edge_rows=True: the row leaves the table and the key
        with it (`events.released`, inside the swap) - the event is unknown again.  `erase`'s limits and refusals carry
        over; no key found: nothing changes and the graph is returned as it is."""
        what = 'retract_events'
        ev = self.events
        if ev is None:
            raise RuntimeError(f'{what}: no event-key tracker is attached (track_events / attach_events)')
        keys = self._device_keys(what, 'keys', keys).reshape(-1)
        found = ev.lookup(keys).long()
        found = found[found > 0]
        if found.numel() == 0:
            return self.graph, found
        return self.erase(eids=found, release_edge_rows=release_edge_rows, keep_from=keep_from), found

    # ---- saving and restoring an online model ----------------------------------------------
    ONLINE_FORMAT, ONLINE_VERSION = 'tiger-online-state', 1
    _MAILBOX = ('node_msg_vals', 'node_msg_ts', 'has_msg_bits')

    def _online_fingerprint(self) -> dict:
        """what a load cannot change: the shapes and choices the modules were constructed with"""
        fg, r = self.raw_feat_getter, getattr(self, 'restarter_fn', None)
        return dict(model=type(self).__name__, dim=int(self.nfeat_dim), efeat_dim=int(self.efeat_dim),
                    has_nfeats=fg.nfeats is not None, has_efeats=fg.efeats is not None, n_layers=int(self.n_layers),
                    n_neighbors=int(self.n_neighbors), n_head=int(self.n_head), msg_src=self.msg_src, upd_src=self.upd_src,
                    msg_tsfm_type=self.msg_tsfm_type, mem_update_type=self.mem_update_type, hit_type=self.hit_type,
                    restarter=None if r is None else type(r).__name__, hist_len=int(getattr(r, 'hist_len', 0)))

    @torch.no_grad()
    def online_state(self) -> dict:
        """Everything a served model is made of, as a dict of CPU tensors and plain values (`torch.save`-able, loadable
        with weights_only=True; the reference - tiger.py, memory.py:127-129, feature_getter.py:41-51 - rebuilds graph,
        mailbox and tables from the data set and has no counterpart): the module's `state_dict()` (parameters, both
        memories with active_mask, restarter), the mailbox's three buffers, the node / edge feature tables with EXACTLY
        their rows (the leading views, not the backing stores; None where the model has none), n_nodes, the graph's
        `state_dict()` and a fingerprint of what a load cannot change.  After `forget` / `release_edge_rows` / `erase` /
        `grow_nodes` none of this can be rebuilt by replaying the stream.  NOT saved: optimiser state, `uptodate` bitmaps,
        CatalogueSnapshots, eids the caller holds.  Refused: a partitioned model (its tables are indexed by row)."""
        self._refuse_partitioned('online_state')
        self._poll_train_errors()
        fg, S = self.raw_feat_getter, self.msg_store
        cpu = lambda t: None if t is None else t.detach().to('cpu', copy=True)
        return dict(format=self.ONLINE_FORMAT, version=self.ONLINE_VERSION, fingerprint=self._online_fingerprint(),
                    n_nodes=int(self.n_nodes), state_dict={k: cpu(v) for k, v in self.state_dict().items()},
                    mailbox={k: cpu(getattr(S, k)) for k in self._MAILBOX},
                    nfeats=cpu(fg.nfeats), efeats=cpu(fg.efeats), graph=self.graph.state_dict())

    def save_online(self, f):
        """`torch.save(self.online_state(), f)`; f: a path or a file object"""
        torch.save(self.online_state(), f)

    @torch.no_grad()
    def load_online(self, f_or_state, *, device=None, verify: bool = True):
        """Become the model that `save_online` / `online_state` saved -> the new graph.  f_or_state: a path, a file object
        or the dict of `online_state`.  The model is one built by the usual constructor on ANY graph and ANY tables of
        the right widths (a fresh process builds it on a stub); device: where the loaded graph lives (default: the
        model's device).  A model that saves at any point of an online run and a freshly built model that loads the file
        continue bit for bit as the uninterrupted model does: embeddings, both memories, mailbox, graph arrays,
        `recommend` lists and 'uniform' draws, through later `observe` / `forget` / `erase` / `release_edge_rows` / growth.
        Everything is checked first: format / version, the fingerprint (dim, widths, n_layers, n_neighbors, n_head,
        msg_src / upd_src, function types, restarter class and hist_len), key set, dtypes and shapes of the saved
        state_dict against the model's (per-node tables may hold more rows), the graph (`Graph.from_state_dict` with the
        rows of the saved edge table: tg_tcsr_verify; verify=False trusts the file's graph), mailbox and table shapes
        against the saved n_nodes, the spare bits of has_msg_bits.  Then: per-node tables grow to the saved n_nodes (the
        `grow_nodes` machinery; its refusals apply - a StaticRestarter model must be built with the saved row count), the
        tables are replaced (`NumericalFeature.install_rows`), state_dict and mailbox are loaded, the graph goes in through
        the setter (the restarter follows) and derived tables and stamps are dropped.  CatalogueSnapshots, captured
        device graphs, StepBuffers and resident runs held from before are stale: the caller's part, as for `forget`.
        Refused before anything changes - IF THE CALL RAISES, EVERY BUFFER, TABLE AND THE GRAPH ARE WHAT THEY WERE: a
        partitioned model, training mode, tables in pinned host memory (register_buffer=False), a stream capture in
        progress, a saved n_nodes below the model's, and every check above (ValueError)."""
        from ..data.graph import Graph
        what = 'load_online'
        self._refuse_partitioned(what)
        self._refuse_tracked(what)
        if self.training:
            raise RuntimeError(f'{what}: an online state is loaded in eval() mode (the streaming state of a served model)')
        fg, S = self.raw_feat_getter, self.msg_store
        if not fg.pin_mem:
            raise NotImplementedError(f'{what}: the feature tables live in pinned host memory (register_buffer=False)')
        if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{what}: tables cannot be replaced while a stream is being captured into a graph')
        st = f_or_state if isinstance(f_or_state, dict) else torch.load(f_or_state, map_location='cpu', weights_only=True)
        if not isinstance(st, dict) or st.get('format') != self.ONLINE_FORMAT:
            raise ValueError(f'{what}: not a saved online state')
        if st.get('version') != self.ONLINE_VERSION:
            raise ValueError(f"{what}: version {st.get('version')!r} of the format is unknown (this library reads "
                             f'{self.ONLINE_VERSION})')
        missing = [k for k in ('fingerprint', 'n_nodes', 'state_dict', 'mailbox', 'nfeats', 'efeats', 'graph') if k not in st]
        if missing:
            raise ValueError(f'{what}: the saved state lacks {missing}')
        chain = st.get('chain')  # (a base of an OnlineJournal carries chain and seq; files without them load as before)
        if chain is not None or st.get('seq') is not None:
            for k in ('chain', 'seq'):
                v = st.get(k)
                if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                    raise ValueError(f'{what}: {k} = {v!r} (a base of a journal carries both as non-negative ints)')
        mine = self._online_fingerprint()
        if st['fingerprint'] != mine:
            theirs = st['fingerprint'] if isinstance(st['fingerprint'], dict) else {}
            diff = {k: (theirs.get(k), v) for k, v in mine.items() if theirs.get(k) != v}
            raise ValueError(f'{what}: the saved model is another model - (saved, this one): {diff}')
        n = st['n_nodes']
        if isinstance(n, bool) or not isinstance(n, int):
            raise ValueError(f'{what}: n_nodes = {n!r}')
        if n < self.n_nodes:
            raise ValueError(f'{what}: the saved model has {n} node ids, this one {self.n_nodes} (node ids are never released: '
                             'build the model on at most the saved count)')
        # -- the state_dict: keys, dtypes, shapes (per-node tables hold the saved count of rows)
        own, sd = self.state_dict(), st['state_dict']
        if not isinstance(sd, dict) or set(sd) != set(own):
            odd = sorted(set(sd) ^ set(own))[:6] if isinstance(sd, dict) else type(sd).__name__
            raise ValueError(f'{what}: the saved state_dict has other keys than the model\'s ({odd})')
        per_node = tuple(f'{m}.{b}' for m in ('left_memory', 'right_memory', 'msg_memory', 'upd_memory')
                         for b in ('vals', 'update_ts', 'active_mask'))
        for k, cur in own.items():
            v = sd[k]
            want = (n,) + tuple(cur.shape[1:]) if k in per_node else tuple(cur.shape)
            if not torch.is_tensor(v) or v.dtype != cur.dtype or tuple(v.shape) != want:
                got = f'{v.dtype} {tuple(v.shape)}' if torch.is_tensor(v) else type(v).__name__
                raise ValueError(f'{what}: state_dict[{k!r}] is {got}, the model wants {cur.dtype} {want}')
        # -- mailbox and tables against the saved count
        mb = st['mailbox']
        shapes = dict(node_msg_vals=(n, S.dim), node_msg_ts=(n,), has_msg_bits=(hip_ops.bitmap_words(n),))
        for k in self._MAILBOX:
            v = mb.get(k) if isinstance(mb, dict) else None
            if not torch.is_tensor(v) or v.dtype != getattr(S, k).dtype or tuple(v.shape) != shapes[k]:
                raise ValueError(f'{what}: mailbox[{k!r}] must be {getattr(S, k).dtype} {shapes[k]}')
        bits = np.unpackbits(mb['has_msg_bits'].contiguous().numpy().view(np.uint8), bitorder='little')
        if bits[n:].any():
            raise ValueError(f'{what}: has_msg_bits marks node id {n + int(np.flatnonzero(bits[n:])[0])}, beyond the saved '
                             f'{n} node ids')
        tables = {}
        for name, cur, rows in (('nfeats', fg.nfeats, n), ('efeats', fg.efeats, None)):
            v = st[name]
            if (v is None) != (cur is None):
                raise ValueError(f'{what}: the saved model has {"a" if v is not None else "no"} {name} table, this one '
                                 f'{"has one" if cur is not None else "none"}')
            if v is None:
                continue
            if (not torch.is_tensor(v) or v.dtype != cur.dtype or v.dim() != 2 or v.shape[1] != cur.shape[1]
                    or (rows is not None and v.shape[0] != rows) or v.shape[0] < 1):
                raise ValueError(f'{what}: the saved {name} table does not fit (width {cur.shape[1]}'
                                 + (f', {rows} rows)' if rows is not None else ')'))
            tables[name] = v
        if n > self.n_nodes:
            self._grow_refusals(what, n, None, None)
        # -- the graph: nothing of it reaches a sampler before tg_tcsr_verify has passed
        dev = self.device if device is None else torch.device(device)
        graph = Graph.from_state_dict(st['graph'], device=dev, verify=verify,
                                      eid_rows=tables['efeats'].shape[0] if 'efeats' in tables else None)
        if graph.num_node != n:
            raise ValueError(f'{what}: the saved graph covers {graph.num_node} node ids, the saved model {n}')
        # -- everything fits: from here on nothing is refused
        if n > self.n_nodes:
            self._grow(n, n - self.n_nodes, None, graph)  # (rows, counts, caches; swaps the graph in through the setter)
        else:
            self.graph = graph
        fg.install_rows(tables.get('nfeats'), tables.get('efeats'))
        self._mark_all('load_online replaced state, graph and tables')
        self.load_state_dict(sd)
        for k in self._MAILBOX:
            getattr(S, k).copy_(mb[k])
        S._version_ += 1
        self._touch()
        self.invalidate_struct()
        # what was derived from the old state, graph or tables, as after a growth
        eager = self._pending is not None
        self._step_ws = {k: v for k, v in self._step_ws.items() if k == 'rng'}
        self._gtab = self._ctab = self._gtab_stamp = None
        self._pending = self._pending_stamp = None
        if eager:
            self.eager_updates()
        if chain is not None:  # a base of a journal: the model is file 0 of that chain, nothing is dirty
            self._journal = OnlineJournal(self)
            self._journal._position(chain, st['seq'])
        return graph

    def _drop_derived(self):
        """what was derived from the old state, graph or tables, as after a growth (the tail of load_online)"""
        self._touch()
        self.invalidate_struct()
        eager = self._pending is not None
        self._step_ws = {k: v for k, v in self._step_ws.items() if k == 'rng'}
        self._gtab = self._ctab = self._gtab_stamp = None
        self._pending = self._pending_stamp = None
        if eager:
            self.eager_updates()

    @torch.no_grad()
    def apply_online_delta(self, f_or_state, *, verify: bool = True):
        """Become the model that wrote the next delta of the journal's chain (`OnlineJournal.save`) -> the new graph.
        f_or_state: a path, a file object or the loaded dict.  Applied once per file, in order, on a model that loaded the
        chain's base with `load_online` (or wrote the files itself): a fresh model that loads the base and applies the
        deltas is, bit for bit, the model that saved them - every tensor of `online_state()`, the graph arrays included,
        and everything it computes afterwards.
        A DELTA IS UNTRUSTED INPUT.  Checked before anything is written, each with a ValueError that names the field:
        format, version, fingerprint, that chain and seq are the expected successor, the "before" counts against the
        model, n_nodes_after >= n_nodes, dtypes and shapes of every tensor, ids and rows strictly ascending inside their
        counts, off[0] == 0 / non-decreasing / off[D] == the packed length.  The new graph is then BUILT beside the old one
        (tg_tcsr_rows_splice: the parent is only read; its one read-back repeats the checks on rows / off and those of the
        old row bounds), must hold num_entry_after entries, and goes through `tg_tcsr_verify` against the NEW edge-table row
        count and its latest time against t_max, before any sampler or table sees it (verify=False skips those two, as in
        `load_online`).  Only then: the tables grow to n_nodes_after (the `grow_nodes` machinery; its refusals apply and are
        made first), the edge-table tail is appended, the state rows are scattered (tg_node_rows_scatter: 8 + 1 tables in
        two launches; tg_bitmap_scatter), the graph goes in through the setter and derived tables and stamps are dropped
        as `load_online` drops them.  The journal then stands at the delta's seq with nothing dirty; a ChangeTracker sees
        the applied ids and rows as changes.  IF THE CALL RAISES, EVERY BUFFER, TABLE AND THE GRAPH ARE WHAT THEY WERE.
        Refused as `load_online`: a partitioned model, training mode, tables in pinned host memory, a stream capture in
        progress; and a model without a journal, or one whose journal is dirty (the model has moved on since the last
        file: it is no longer the delta's predecessor)."""
        what = 'apply_online_delta'
        self._refuse_partitioned(what)
        self._refuse_tracked(what)
        if self.training:
            raise RuntimeError(f'{what}: a delta is applied in eval() mode (the streaming state of a served model)')
        fg, S, J = self.raw_feat_getter, self.msg_store, self._journal
        if not fg.pin_mem:
            raise NotImplementedError(f'{what}: the feature tables live in pinned host memory (register_buffer=False)')
        if self.device.type != 'cuda':
            raise RuntimeError(f'{what}: the model lives on {self.device}; deltas are applied on the GPU')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{what}: tables cannot be written while a stream is being captured into a graph')
        st = f_or_state if isinstance(f_or_state, dict) else torch.load(f_or_state, map_location='cpu', weights_only=True)
        if not isinstance(st, dict) or st.get('format') != OnlineJournal.DELTA_FORMAT:
            raise ValueError(f'{what}: format - not a saved online delta')
        if st.get('version') != OnlineJournal.DELTA_VERSION:
            raise ValueError(f"{what}: version {st.get('version')!r} of the format is unknown (this library reads "
                             f'{OnlineJournal.DELTA_VERSION})')
        counts = ('n_nodes', 'graph_nodes', 'num_entry', 'efeat_rows')
        keys = ('chain', 'seq', 'fingerprint', 'ids', 'rows_of', 'has_msg', 'efeats_tail', 'rows', 'off', 'ts', 'nbr', 'eid',
                'graph_state') + tuple(f'{c}_{w}' for c in counts for w in ('before', 'after'))
        missing = [k for k in keys if k not in st]
        if missing:
            raise ValueError(f'{what}: the delta lacks {missing}')
        mine = self._online_fingerprint()
        if st['fingerprint'] != mine:
            theirs = st['fingerprint'] if isinstance(st['fingerprint'], dict) else {}
            diff = {k: (theirs.get(k), v) for k, v in mine.items() if theirs.get(k) != v}
            raise ValueError(f'{what}: fingerprint - the delta is of another model - (saved, this one): {diff}')
        isint = lambda v: isinstance(v, int) and not isinstance(v, bool)
        for k in ('chain', 'seq') + tuple(f'{c}_{w}' for c in counts for w in ('before', 'after')):
            if not isint(st[k]) or st[k] < 0:
                raise ValueError(f'{what}: {k} = {st[k]!r}')
        if J is None or J.chain is None:
            raise ValueError(f'{what}: chain - this model follows no chain (load the base with load_online first)')
        if st['chain'] != J.chain:
            raise ValueError(f"{what}: chain {st['chain']} is not the chain this model follows ({J.chain})")
        if st['seq'] != J.seq + 1:
            raise ValueError(f"{what}: seq {st['seq']} is not the successor of the file this model stands at ({J.seq})")
        if J.whole or J.saved is None:
            raise ValueError(f'{what}: seq - the model has left the chain since file {J.seq} ({J.reason}); load a base')
        g_old = self.graph
        g_old.tcsr  # (a graph that was never sampled from has no device arrays yet)
        rows_now = 0 if fg.efeats is None else int(fg.efeats.shape[0])
        have = dict(n_nodes=int(self.n_nodes), graph_nodes=int(g_old.num_node), num_entry=int(g_old.tcsr.num_entry),
                    efeat_rows=rows_now)
        for c in counts:
            if st[f'{c}_before'] != have[c]:
                raise ValueError(f"{what}: {c}_before = {st[f'{c}_before']}, but the model has {have[c]}")
        n0, n1 = have['n_nodes'], st['n_nodes_after']
        gn1, P1, er1 = st['graph_nodes_after'], st['num_entry_after'], st['efeat_rows_after']
        if n1 < n0 or n1 > 0x7FFFFFFF:
            raise ValueError(f'{what}: n_nodes_after = {n1} is below the model\'s {n0} (node ids are never released)')
        if gn1 < have['graph_nodes'] or gn1 > n1:
            raise ValueError(f"{what}: graph_nodes_after = {gn1} is outside [{have['graph_nodes']}, {n1}]")
        if er1 < rows_now or P1 > 0xFFFFFFFF:
            raise ValueError(f'{what}: efeat_rows_after = {er1} / num_entry_after = {P1} do not fit')
        # -- dtypes and shapes

        def tensor(name, v, dtype, shape):
            if not torch.is_tensor(v) or v.dtype != dtype or tuple(v.shape) != tuple(shape):
                got = f'{v.dtype} {tuple(v.shape)}' if torch.is_tensor(v) else type(v).__name__
                raise ValueError(f'{what}: {name} is {got}, wanted {dtype} {tuple(shape)}')
            return v.contiguous()

        def ascending(name, v, hi):
            if v.numel() and (int(v[0]) < 0 or int(v[-1]) >= hi or bool((v[1:] <= v[:-1]).any())):
                raise ValueError(f'{what}: {name} must ascend strictly inside [0, {hi})')

        ids = st['ids']
        D = int(ids.numel()) if torch.is_tensor(ids) and ids.dim() == 1 else -1
        ids = tensor('ids', ids, torch.int32, (max(D, 0),))
        ascending('ids', ids, n1)
        tables = OnlineJournal.per_node_tables(self)
        packed = st['rows_of']
        if not isinstance(packed, dict) or set(packed) != set(tables):
            raise ValueError(f'{what}: rows_of must hold the rows of {sorted(tables)}')
        packed = {k: tensor(f'rows_of[{k!r}]', packed[k], t.dtype, (D,) + tuple(t.shape[1:])) for k, t in tables.items()}
        has = tensor('has_msg', st['has_msg'], torch.uint8, (D,))
        tail = st['efeats_tail']
        if (tail is None) != (fg.efeats is None):
            raise ValueError(f'{what}: efeats_tail - the delta has {"a" if tail is not None else "no"} edge table, this model '
                             f'{"has one" if fg.efeats is not None else "none"}')
        if tail is not None:
            tail = tensor('efeats_tail', tail, fg.efeats.dtype, (er1 - rows_now, fg.efeats.shape[1]))
        elif er1 != rows_now:
            raise ValueError(f'{what}: efeat_rows_after = {er1} for a model without an edge table')
        rows = st['rows']
        Dg = int(rows.numel()) if torch.is_tensor(rows) and rows.dim() == 1 else -1
        rows = tensor('rows', rows, torch.int32, (max(Dg, 0),))
        ascending('rows', rows, gn1)
        off = tensor('off', st['off'], torch.int64, (Dg + 1,))
        n_pack = int(st['ts'].numel()) if torch.is_tensor(st['ts']) and st['ts'].dim() == 1 else -1
        pack = tuple(tensor(k, st[k], dt, (max(n_pack, 0),))
                     for k, dt in (('ts', torch.float64), ('nbr', torch.int32), ('eid', torch.int32)))
        if int(off[0]) != 0 or bool((off[1:] < off[:-1]).any()) or int(off[-1]) != n_pack:
            raise ValueError(f'{what}: off must start at 0, never decrease and end at the packed length {n_pack}')
        if have['num_entry'] + n_pack > 0xFFFFFFFF:
            raise ValueError(f'{what}: ts - {n_pack} packed entries beside {have["num_entry"]} are more than a T-CSR holds')
        gs = st['graph_state']
        gkeys = ('t_last', 'time_ordered', 'rng_kind', 'rng_key', 'rng_pos', 'rng_has_gauss', 'rng_cached_gaussian', 'mt_state')
        if not isinstance(gs, dict) or any(k not in gs for k in gkeys):
            raise ValueError(f'{what}: graph_state must hold {gkeys}')
        key, mt = gs['rng_key'], gs['mt_state']
        if (not isinstance(gs['t_last'], float) or not isinstance(gs['time_ordered'], bool) or gs['rng_kind'] != 'MT19937'
                or not torch.is_tensor(key) or key.dtype != torch.int64 or tuple(key.shape) != (624,) or int(key.min()) < 0
                or int(key.max()) > 0xFFFFFFFF or not isint(gs['rng_pos']) or not 0 <= gs['rng_pos'] <= 624
                or not isint(gs['rng_has_gauss']) or not isinstance(gs['rng_cached_gaussian'], float)):
            raise ValueError(f'{what}: graph_state holds no latest time, time-ordered flag and MT19937 state')
        if mt is not None and (not torch.is_tensor(mt) or mt.dtype != torch.int32 or tuple(mt.shape) != (625,)
                               or not 0 <= int(mt[624]) <= 624):
            raise ValueError(f'{what}: graph_state[\'mt_state\'] is no int32 [625] device MT19937 state')
        if n1 > n0:
            self._grow_refusals(what, n1, None, None)
        # -- the new graph, built beside the old one: nothing of it reaches a sampler or a table before it has passed
        dev = self.device
        up = lambda t: t.to(dev)
        code, first, arrays = hip_ops.tcsr_rows_splice(g_old, gn1, up(rows), up(off), tuple(up(t) for t in pack), strict=False)
        if code:
            field = ('rows', 'off', 'the model\'s own graph')[code - 1]
            raise ValueError(f'{what}: {field} - ' + hip_ops.SPLICE_TEXT(code, first))
        if int(arrays[1].numel()) != P1:
            raise ValueError(f'{what}: num_entry_after = {P1}, but the spliced graph holds {arrays[1].numel()} entries')
        if verify:
            vcode, vfirst, t_max = hip_ops.tcsr_verify(arrays, er1 if fg.efeats is not None else None)
            if vcode:
                raise ValueError(f'{what}: the spliced graph is ' + hip_ops.TCSR_VERIFY_TEXT(vcode, vfirst))
            if not gs['t_last'] >= t_max:
                raise ValueError(f"{what}: graph_state['t_last'] = {gs['t_last']} is below the largest time of the entries "
                                 f'({t_max})')
        child = g_old._child(num_node=gn1)
        child.rng = np.random.RandomState()
        child.rng.set_state((str(gs['rng_kind']), key.numpy().astype(np.uint32), int(gs['rng_pos']), int(gs['rng_has_gauss']),
                             float(gs['rng_cached_gaussian'])))
        child._time_ordered, child._t_last, child._mt_saved = bool(gs['time_ordered']), float(gs['t_last']), None
        child._adopt_device(arrays)
        child._mt = None if mt is None else mt.to(dev).contiguous()
        ids_d, has_d = up(ids), up(has)
        packed = {k: up(v) for k, v in packed.items()}
        tail = None if tail is None else up(tail)
        # -- everything fits and everything is built: from here on nothing is refused
        if n1 > n0:
            self._grow(n1, n1 - n0, None, g_old)
            tables = OnlineJournal.per_node_tables(self)  # (the grown views)
        if tail is not None and tail.shape[0] and fg.append_edge_rows(tail):
            self.invalidate_struct()
        if D:
            pairs = [(packed[k], t) for k, t in tables.items()]
            for i in range(0, len(pairs), hip_ops._lib.TG_NODE_ROWS_MAX):
                hip_ops.node_rows_scatter(pairs[i:i + hip_ops._lib.TG_NODE_ROWS_MAX], ids_d)
            hip_ops.bitmap_scatter(has_d, ids_d, S.has_msg_bits, n1)
            for mod in (self.left_memory, self.right_memory, S):
                mod._version_ += 1
            fg._version_ = getattr(fg, '_version_', 0) + 1
            fg._nz_cache = None
            if self._tracker is not None:
                self._tracker.mark(ids_d)
        self.graph = child  # (the setter: the restarter follows; a tracker marks the rows whose length changed)
        if self._tracker is not None and Dg:
            self._tracker.mark(up(rows))  # (a row rewritten at its old length too)
        self._drop_derived()
        J._position(st['chain'], st['seq'])
        return child

    # ---- remaining reference methods -----------------------------------------------------
    @torch.no_grad()
    def update_right_memory(self, node_ids: Tensor, new_vals: Tensor, ts: Tensor):
        self.right_memory.set(node_ids, new_vals, ts)
        self._mark(node_ids)

    @torch.no_grad()
    def update_left_memory(self, node_ids: Tensor, new_vals: Tensor, ts: Tensor):
        node_ids, index = select_latest_nids(node_ids, ts, self.n_nodes)
        self.left_memory.set(node_ids, new_vals[index], ts[index])
        self._mark(node_ids)

    @torch.no_grad()
    def flush_msg(self):
        """tiger.py:444-455: consume every pending message into the right memory."""
        self._refuse_partitioned('flush_msg')
        self._poll_train_errors()
        self._touch()
        self._mark_all('flush_msg consumed every pending message')
        dev = self.device
        m = self.model_struct()
        err = hip_ops.new_err(dev)
        bits = self.msg_store.has_msg_bits
        comp, reprs = self._consume(bits, self.n_nodes, err)  # involved == outdated == all pending nodes
        n = int(comp['count'].item())
        if n:
            ids = comp['ids'][:n]
            mts = self.msg_store.node_msg_ts[ids]
            self.right_memory.set(ids, reprs[:n], mts)
            self.msg_store.clear(ids)
        hip_ops.raise_if_err(err)

    def load_state_dict(self, *args, **kwargs):
        """parameters (and memories) change under the derived tables: the pre-multiplied attention weights are
        recomputed and the eager-update table is rebuilt before its next use"""
        out = super().load_state_dict(*args, **kwargs)
        self._touch()
        self._mark_all('load_state_dict replaced parameters and memories')
        if self._fused is not None:
            self.fuse_attention()
        return out

    def reset(self):
        self._touch()
        self._mark_all('reset cleared every memory and the mailbox')
        self.left_memory.clear()
        self.right_memory.clear()
        self.msg_store.clear()

    def save_memory_state(self):
        return (self.left_memory.clone(), self.right_memory.clone(), self.msg_store.clone())

    def load_memory_state(self, data):
        for new, cur in zip(data, (self.left_memory, self.right_memory, self.msg_store)):
            if new.n != cur.n:  # (a state saved before grow_nodes: the structs would address rows it does not have)
                raise ValueError(f'load_memory_state: the saved state holds {new.n} rows per table, the model {cur.n} '
                                 '(saved before grow_nodes admitted node ids? grow it with its own grow(n) first)')
        self._touch()
        self._mark_all('load_memory_state replaced every memory and the mailbox')
        self.left_memory, self.right_memory, self.msg_store = data
        self.msg_memory = self.left_memory if self.msg_src == 'left' else self.right_memory
        self.upd_memory = self.left_memory if self.upd_src == 'left' else self.right_memory
        self._struct_cache = None


class TIGER(TIGE):
    def __init__(self, *, raw_feat_getter, graph, restarter, n_neighbors: int = 20, n_layers: int = 2,
                 n_head: int = 2, dropout: float = 0.1, msg_src: str, upd_src: str, msg_tsfm_type: str = 'id',
                 mem_update_type: str = 'gru', tgn_mode: bool = True, msg_last_only: bool = True,
                 hit_type: str = 'vec'):
        super().__init__(raw_feat_getter=raw_feat_getter, graph=graph, n_neighbors=n_neighbors, n_layers=n_layers,
                         n_head=n_head, dropout=dropout, msg_src=msg_src, upd_src=upd_src,
                         msg_tsfm_type=msg_tsfm_type, mem_update_type=mem_update_type, tgn_mode=tgn_mode,
                         msg_last_only=msg_last_only, hit_type=hit_type)
        self.restarter_fn = restarter
        self.restarter_fn.model_struct_fn = self.model_struct
        self.restarter_fn.rng_fn = self.dropout_rng
        self.mutual_loss_fn = nn.MSELoss()

    def forward(self, *args, **kwargs):
        return self.contrast_and_mutual_learning(*args, **kwargs)

    def contrast_and_mutual_learning(self, src_ids, dst_ids, neg_dst_ids, ts, eids, computation_graph,
                                     contrast_only: bool = False):
        """tiger.py:547-592"""
        if self.training and torch.is_grad_enabled():
            losses, *_ = self._train_forward(src_ids, dst_ids, neg_dst_ids, ts, eids, computation_graph,
                                             mutual=not contrast_only)
            if contrast_only:
                return losses[0], torch.zeros((), dtype=torch.int64, device=losses.device)  # no host copy
            return losses[0], losses[1]
        with torch.no_grad():
            return self._contrast_and_mutual_eval(src_ids, dst_ids, neg_dst_ids, ts, eids, computation_graph,
                                                  contrast_only)

    def _contrast_and_mutual_eval(self, src_ids, dst_ids, neg_dst_ids, ts, eids, computation_graph,
                                  contrast_only: bool = False):
        contrast_loss, *_, h_prev_left, h_prev_right = self.contrast_learning(
            src_ids, dst_ids, neg_dst_ids, ts, eids, computation_graph)
        if contrast_only:
            return contrast_loss, torch.zeros((), dtype=torch.int64, device=contrast_loss.device)
        dev = self.device
        index = computation_graph.restart_data.index
        unique_nids = torch.cat([src_ids, dst_ids]).to(dev)[index]
        unique_ts = ts.to(dev).float().repeat(2)[index]
        sur_left, sur_right, _ = self.restarter_fn(unique_nids, unique_ts, computation_graph)
        targets = torch.cat([h_prev_left[index], h_prev_right[index]], 0)
        preds = torch.cat([sur_left, sur_right], 0)
        valid_rows = torch.where(~(targets == 0).all(1))[0]
        if len(valid_rows):
            mutual_loss = self.mutual_loss_fn(preds[valid_rows], targets[valid_rows])
        else:
            mutual_loss = torch.zeros((), dtype=torch.int64, device=dev)
        return contrast_loss, mutual_loss

    @torch.no_grad()
    def restart(self, nids: Tensor, ts: Tensor, mix: float = 0.):
        """tiger.py:594-609: fill both memories with the surrogate state."""
        self._refuse_partitioned('restart')
        if len(nids) == 0:
            return
        self._touch()
        dev = self.device
        nids = nids.to(dev).long().contiguous()
        self._mark(nids)
        h_left, h_right, prev_ts = self.restarter_fn(nids, ts.to(dev))
        if mix > 0:
            # the library's gather, not torch indexing: tables beyond 2^31 elements (10 M nodes x 256)
            h_left = mix * h_left + (1 - mix) * hip_ops.gather_rows(self.left_memory.vals, nids)
            h_right = mix * h_right + (1 - mix) * hip_ops.gather_rows(self.right_memory.vals, nids)
        m = self.model_struct()
        check(lib.tg_restart_apply(C.byref(m), nids.numel(), ptr(nids), ptr(h_left.contiguous()),
                                   ptr(h_right.contiguous()), ptr(prev_ts.contiguous()), stream_ptr(dev)),
              'tg_restart_apply')

    @torch.no_grad()
    def restart_involved(self, nodes: Tensor, ts: Tensor, uptodate: Tensor, *, graph=None) -> int:
        """The lazy restart of eval_utils.py:37-42 for a flat list of (node, time) queries that are about to be embedded:
        every node their embeddings will read (the queries, their sampled neighbours, on a two-layer model the neighbours'
        neighbours - the set GraphCollator.collate_memory_nodes flags) that the bitmap `uptodate` (hip_ops.new_bitmap) does
        not hold yet is restarted at the earliest query time and marked in the bitmap -> how many were restarted (also
        kept in `last_restarted`).  One listing call (tg_involved_list: no neighbour list is written), one read-back of the
        count, then `restart_list` on the device-resident list (SeqRestarter: one library call; anything else: `restart`);
        per-node tables of a model with eager updates that were current stay current.  graph: the graph the embeddings
        will sample from (default: model.graph).  eval() mode only.  Refused before anything runs, with state and bitmap
        untouched: a partitioned model, training mode, strategy 'uniform', a graph of another size, an id outside
        [0, n_nodes)."""
        self._refuse_partitioned('restart_involved')
        if self.training:
            raise RuntimeError('restart_involved restarts for scoring in eval() mode')
        graph = self.graph if graph is None else graph
        strategy = getattr(graph, 'strategy', 'recent_edges')
        if strategy not in ('recent_edges', 'recent_nodes'):
            raise NotImplementedError(f"restart_involved lists 'recent_edges' or 'recent_nodes' neighbourhoods; strategy="
                                      f"{strategy!r} would make the set depend on the graph's random stream")
        self.check_graph(graph)
        self._check_uptodate('restart_involved', uptodate)
        dev = self.device
        nodes = torch.as_tensor(nodes).to(dev).long().contiguous().reshape(-1)
        ts64 = torch.as_tensor(ts).to(dev).double().contiguous().reshape(-1)
        out = hip_ops.involved_list(graph, nodes, ts64, self.n_neighbors, self.n_layers, uptodate, strategy=strategy)
        n = self.last_restarted = int(out['count'].item())
        if n:
            self.restart_list_keep_tables(out['ids'][:n], out['tmin'])
        return n

    @property
    def graph(self):
        return self.temporal_embedding_fn.graph

    @graph.setter
    def graph(self, new_obj):
        old = self.temporal_embedding_fn.graph
        self.temporal_embedding_fn.graph = new_obj
        self.restarter_fn.graph = new_obj
        for sink in self._sinks():
            sink.mark_graph(old, new_obj)
