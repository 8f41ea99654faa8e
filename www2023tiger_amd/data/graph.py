"""Temporal graph with a device-resident time-sorted CSR (T-CSR).

Mirror of tiger/data/graph.py (`Graph`): same constructor, `from_data`,
`num_node`, `sample_temporal_neighbor` and `get_history` signatures and return
types, but the per-query Python loop (graph.py:94-146, "Bottleneck! Total time
>50%") is replaced by HIP kernels over the T-CSR (csrc/tg_graph.hip).

The object is immutable after construction, so the collator thread and the main
thread may sample concurrently (each call allocates its own outputs and runs on
the calling thread's current stream).  New events are ingested by `extended`, which
returns a NEW Graph (csrc/tg_append.hip) and leaves its parent as it was; late events - a batch in any order, at any
times - by `merged`, which does the same (tg_tcsr_merge, same file); old entries
are dropped by `trimmed` (csrc/tg_trim.hip), which does the same, `without` takes particular nodes and events out
(csrc/tg_erase.hip), `renumbered` gives the entries the row numbers of a packed edge table (csrc/tg_edge_rows.hip), and
`compacted` renumbers the node ids densely without the erased ones (csrc/tg_node_compact.hip).
"""
import ctypes as C
import itertools
import operator
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .._lib import TgTcsr, check, lib, ptr
from ..hip_ops import stream_ptr, tcsr_arrays, tcsr_compacted, tcsr_compacted_host


class _HostRoot:
    """Host-side origin of a graph: the events of from_arrays and / or the host T-CSR arrays.  Shared by reference along a
    chain of `extended` graphs until one of them materialises its own host view."""
    __slots__ = ('events', 'host', 'dev', 'num_node')

    def __init__(self, num_node):
        self.num_node = num_node  # ids the host arrays cover (a chain that admitted new ids covers more than its root)
        self.events = None  # (src, dst, ts, eids) of from_arrays, the input of either builder
        self.host = None    # host T-CSR arrays (indptr, ts, nbr, eid), built on demand
        self.dev = None     # a graph trimmed on the device: its device arrays, which `host` is downloaded from on demand


_SERIAL = itertools.count(1)  # process-wide: next() is atomic under the GIL


class Graph:
    def __init__(self, adj_list, strategy='recent_nodes', seed=None, alpha=0.0, device=None):
        """adj_list[n] = list of (neighbor, edge_index, timestamp, is_dst_flag), as built by
        the reference's data2adjlist (graph.py:226-241).  Prefer `from_data` /
        `from_arrays`, which never materialise Python tuples."""
        owner, nbr, eid, ts, flag = [], [], [], [], []
        for n, edges in enumerate(adj_list):
            for (o, e, t, f) in edges:
                owner.append(n)
                nbr.append(o)
                eid.append(e)
                ts.append(t)
                flag.append(f)
        owner = np.asarray(owner, dtype=np.int64)
        ts = np.asarray(ts, dtype=np.float64)
        order = np.lexsort((np.arange(len(owner)), ts, owner))  # stable sort by time inside a node (graph.py:32)
        eid = np.asarray(eid, dtype=np.int64)
        if len(eid) and (eid.min() < 0 or eid.max() > 0x7FFFFFFF):
            raise ValueError('edge ids must fit in 31 bits')
        self._init_common(len(adj_list), strategy, seed, alpha, device)
        self._t_last = float(ts.max()) if len(ts) else -np.inf
        packed = eid[order].astype(np.uint32) | (np.asarray(flag, dtype=np.uint32)[order] << np.uint32(31))
        self._host = (np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=self.num_node))]).astype(np.int64),
                      ts[order], np.asarray(nbr, dtype=np.int64)[order].astype(np.int32), packed.view(np.int32))

    def _init_common(self, num_node, strategy, seed, alpha, device, rng=None):
        self.num_node = int(num_node)
        self.strategy = strategy
        self.seed = seed
        self.alpha = alpha
        # graph.py:22; its state seeds the device MT19937 (rng: an extended graph continues its parent's stream)
        self.rng = np.random.RandomState(seed) if rng is None else rng
        self._device = torch.device(device) if device is not None else None
        self._dev = None  # device tensors, built / uploaded lazily
        self._mt = None
        self._mt_saved = None  # a host graph of `from_state_dict`: the saved device MT19937 state, uploaded on first use
        self._root = _HostRoot(self.num_node)  # the host view: `_events`, `_host` below
        self._log = None     # extended graphs: (parent's log, batch) - the batches appended to the root, newest first
        self._time_ordered = False
        self._t_last = -np.inf  # latest event time, kept on the host (a 0-d device tensor after an unvalidated device batch)
        self.serial = next(_SERIAL)  # a struct's address can be reused after its graph died; a serial number cannot
        self.last_batch = None  # extended graphs: the (src, dst, ts, eids) they were extended by - device tensors when that
                                # happened on the device, so a caller that streams the same batch next need not upload it again

    # the host view is produced lazily for an extended graph (the device path of `extended` touches no host array)
    @property
    def _events(self):
        self._materialise()
        return self._root.events

    @_events.setter
    def _events(self, value):
        self._root.events = value

    @property
    def _host(self):
        return self._root.host if self._log is None else None

    @_host.setter
    def _host(self, value):
        self._root.host = value

    def _materialise(self):
        """fold the appended batches into a host view of this graph's own: the root's events followed by the batches, and
        the root's host T-CSR extended by them (tg_tcsr_append_host: what the host builder gives over the concatenation)"""
        if self._log is None:
            return
        batches, node = [], self._log
        while node is not None:  # (a loop: a chain may be thousands of batches long)
            node, b = node
            batches.append(b)
        batches.reverse()
        to_np = lambda x, dt: np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=dt)
        src, dst, ts, eids = (np.concatenate([to_np(b[i], dt) for b in batches])
                              for i, dt in enumerate((np.int64, np.int64, np.float64, np.int64)))
        old, new = self._root, _HostRoot(self.num_node)
        if old.events is not None:
            new.events = tuple(np.concatenate([a, b]) for a, b in zip(old.events, (src, dst, ts, eids)))
        if old.host is not None or old.events is None or not self._time_ordered:
            self._host_of(old)
            n = len(src)
            h = tcsr_arrays(self.num_node, len(old.host[1]) + 2 * n)
            # (the root may cover fewer ids than this graph: a chain that admitted new ones - `extended(num_node=)`)
            g = TgTcsr(old.num_node, len(old.host[1]), *(ptr(a) for a in old.host))
            check(lib.tg_tcsr_append_grow_host(C.byref(g), self.num_node, n, ptr(src), ptr(dst), ptr(ts), ptr(eids),
                                               *(ptr(a) for a in h)), 'tg_tcsr_append_grow_host')
            new.host = h
        self._root, self._log = new, None

    @classmethod
    def from_arrays(cls, src, dst, ts, eids, strategy='recent_nodes', seed=None, max_node_id=None, device=None):
        src = np.ascontiguousarray(src, dtype=np.int64)
        dst = np.ascontiguousarray(dst, dtype=np.int64)
        ts = np.ascontiguousarray(ts, dtype=np.float64)
        eids = np.ascontiguousarray(eids, dtype=np.int64)
        if max_node_id is None:
            max_node_id = int(max(src.max(), dst.max()))
        self = cls.__new__(cls)
        self._init_common(max_node_id + 1, strategy, seed, 0.0, device)
        E = len(src)
        if E and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= self.num_node):
            raise ValueError('node ids must lie in [0, num_node)')
        if E and (eids.min() < 0 or eids.max() > 0x7FFFFFFF):
            raise ValueError('edge ids must fit in 31 bits')
        self._events = (src, dst, ts, eids)
        self._t_last = float(ts.max()) if E else -np.inf
        # a time-ordered stream (every JODIE file) is built on the GPU; others take the host builder,
        # which also performs the reference's stable per-node sort by time (graph.py:32)
        self._time_ordered = bool(E < 2 or np.all(ts[1:] >= ts[:-1])) and 2 * E < 2 ** 32
        return self

    def _build_host(self, events, num_node):
        src, dst, ts, eids = events
        E = len(src)
        h = tcsr_arrays(num_node, 2 * E)
        check(lib.tg_tcsr_build_host(E, ptr(src), ptr(dst), ptr(ts), ptr(eids), num_node, *(ptr(a) for a in h)),
              'tg_tcsr_build_host')
        return h

    def _host_of(self, root):
        """the host T-CSR arrays of a root: built from its events, or (a graph trimmed on the device has no event list)
        downloaded from its device arrays"""
        if root.host is None:
            if root.dev is not None:
                root.host = tuple(np.ascontiguousarray(t.cpu().numpy()) for t in root.dev)
            else:
                root.host = self._build_host(root.events, root.num_node)
        root.dev = None
        return root.host

    def _host_tcsr(self):
        self._materialise()
        return self._host_of(self._root)

    _h_indptr = property(lambda self: self._host_tcsr()[0])
    _h_ts = property(lambda self: self._host_tcsr()[1])
    _h_nbr = property(lambda self: self._host_tcsr()[2])
    _h_eid = property(lambda self: self._host_tcsr()[3])

    def _build_on_device(self, dev):
        src, dst, ts, eids = (torch.from_numpy(a).to(dev) for a in self._events)
        E = src.numel()
        out = tcsr_arrays(self.num_node, 2 * E, dev)
        nbytes = int(lib.tg_tcsr_build_device_workspace_bytes(E, self.num_node))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib.tg_tcsr_build_device(E, ptr(src), ptr(dst), ptr(ts), ptr(eids), self.num_node, *(ptr(t) for t in out),
                                           ptr(ws), nbytes, stream_ptr(dev)), 'tg_tcsr_build_device')
            torch.cuda.current_stream(dev).synchronize()  # the inputs and the workspace die with this scope
        return out

    @classmethod
    def from_data(cls, data, strategy='recent_nodes', seed=None, max_node_id=None, device=None):
        """`data` is an InteractionData-like object with .src/.dst/.ts/.eids arrays (graph.py:38-42)."""
        return cls.from_arrays(data.src, data.dst, data.ts, data.eids, strategy=strategy, seed=seed,
                               max_node_id=max_node_id, device=device)

    # ---- device residency ---------------------------------------------------------
    @property
    def device(self) -> torch.device:
        if self._device is None:
            self._device = torch.device('cuda', torch.cuda.current_device())
        return self._device

    def to(self, device):
        device = torch.device(device)
        if self._device != device:
            self._device, self._dev, self._mt = device, None, None
        return self

    def _tensors(self):
        if self._dev is None:
            dev = self.device
            if self._time_ordered and self._events is not None and self._host is None:
                self._dev = self._build_on_device(dev)  # tg_tcsr_build_device: stable radix sort on the owner id
            else:
                self._dev = tuple(torch.from_numpy(a).to(dev) for a in self._host_tcsr())
            self._set_struct()
        return self._dev

    def _set_struct(self):
        self._struct = TgTcsr(self.num_node, self._dev[1].numel(), *[t.data_ptr() for t in self._dev])
        self._struct.serial = self.serial  # (TIGE._prefetch_stamp: which graph a struct belongs to)

    @property
    def tcsr(self) -> TgTcsr:
        self._tensors()
        return self._struct

    def _mt_state(self) -> Tensor:
        if self._mt is None and self._mt_saved is not None:
            self._mt = self._mt_saved.to(self.device)
        if self._mt is None:
            _, key, pos, _, _ = self.rng.get_state()
            st = np.concatenate([key.astype(np.uint32), np.array([pos], dtype=np.uint32)]).view(np.int32)
            self._mt = torch.from_numpy(st.copy()).to(self.device)
        return self._mt

    # ---- deriving a graph from a graph ------------------------------------------------
    def _child(self, num_node=None) -> 'Graph':
        """A NEW Graph that carries this one over: strategy / seed / alpha / device, the SAME `rng` object, the time-ordered
        flag and the latest event time; num_node unless overridden (`extended`); a serial of its own and no arrays yet."""
        child = Graph.__new__(Graph)
        child._init_common(self.num_node if num_node is None else num_node, self.strategy, self.seed, self.alpha, self._device,
                           rng=self.rng)
        child._time_ordered = self._time_ordered
        child._t_last = self._t_last
        child._mt_saved = self._mt_saved
        return child

    def _adopt_device(self, arrays, parent: Optional['Graph'] = None) -> 'Graph':
        """Make the device arrays this graph's own (host view: downloaded on first use); the MT19937 state is the parent's."""
        self._dev = self._root.dev = tuple(arrays)
        self._set_struct()
        if parent is not None:
            self._mt = parent._mt_state()
        return self

    def _adopt_host(self, arrays, events, parent: 'Graph') -> 'Graph':
        """Make the host arrays this graph's own, and `events` (if not None) the event list they are the T-CSR of.  The
        device MT19937 state is the parent's IF IT HAS ONE, else None: derived from the shared `rng` on first use.  (The child of
        `extended` adopts nothing - it shares `_root` and `_log` - and takes that state on the device path only, never here.)"""
        self._host = tuple(arrays)
        if events is not None:
            self._events = events
        if parent._mt is not None:
            self._mt = parent._mt
        return self

    @classmethod
    def _from_device_arrays(cls, arrays, t_last, time_ordered: bool, strategy='recent_nodes', seed=None) -> 'Graph':
        """a device-resident Graph over T-CSR arrays built on their device (no event list, as a graph trimmed there)"""
        self = cls.__new__(cls)
        self._init_common(arrays[0].numel() - 1, strategy, seed, 0.0, arrays[0].device)
        self._time_ordered, self._t_last = bool(time_ordered), t_last
        return self._adopt_device(arrays)

    # ---- saving and restoring -------------------------------------------------------
    STATE_FORMAT, STATE_VERSION = 'tiger-graph', 1

    def state_dict(self) -> dict:
        """This graph as a flat dict of CPU tensors and plain Python values (`torch.save`, `torch.load(weights_only=True)`;
        graph.py:11-42 has no counterpart: the reference rebuilds its graph from the data set).  The four arrays of THIS
        graph - a chain child of `extended` as well as a child of `trimmed` / `without` / `renumbered`, copied from the
        device for a device-resident graph, from the host view otherwise -, num_node, the latest event time (a 0-d device
        value is resolved: one read-back), the time-ordered flag, strategy / seed / alpha, the state of `rng` and, if the
        graph has one, the device MT19937 state.  Not saved: the event list and `last_batch`."""
        if self._dev is not None:
            arrays = tuple(t.detach().to('cpu', copy=True) for t in self._dev)
        else:
            arrays = tuple(torch.from_numpy(np.array(a, copy=True)) for a in self._host_tcsr())
        kind, key, pos, has_gauss, gauss = self.rng.get_state()
        sd = dict(format=self.STATE_FORMAT, version=self.STATE_VERSION,
                  indptr=arrays[0], ts=arrays[1], nbr=arrays[2], eid=arrays[3], num_node=int(self.num_node),
                  t_last=float(self._t_last), time_ordered=bool(self._time_ordered),
                  strategy=self.strategy, seed=None if self.seed is None else int(self.seed), alpha=float(self.alpha),
                  rng_kind=str(kind), rng_key=torch.from_numpy(key.astype(np.int64)), rng_pos=int(pos),
                  rng_has_gauss=int(has_gauss), rng_cached_gaussian=float(gauss),
                  mt_state=None if self._mt is None else self._mt.detach().to('cpu', copy=True))
        return sd

    @classmethod
    def from_state_dict(cls, sd: dict, device=None, verify: bool = True, eid_rows: Optional[int] = None) -> 'Graph':
        """The root Graph a `state_dict` describes.  device: where it lives - device-resident there (its host view is
        downloaded on first use); None: the current GPU, or a host graph when there is none (as with device='cpu').  `rng` is
        restored with `set_state` and the device MT19937 state is the saved one, so 'uniform' draws continue the saved
        stream; the graph has a `serial` of its own and no event list.
        verify=True refuses, BEFORE any array reaches a sampler (ValueError): an unknown format / version, arrays of other
        dtypes or shapes, lengths that do not fit each other or num_node, any non-zero code of `hip_ops.tcsr_verify` (the
        host twin without a device; the message names class and index: TCSR_VERIFY_TEXT), with eid_rows an edge id that is
        no row of the caller's edge table, and a saved latest time BELOW the largest time of the arrays.  (ABOVE is legal:
        `trimmed` / `without` carry the parent's latest time on purpose.)  verify=False trusts the caller, as
        `extended(validate=False)` does."""
        from .. import hip_ops
        if not isinstance(sd, dict) or sd.get('format') != cls.STATE_FORMAT:
            raise ValueError(f"from_state_dict: not a saved graph (format {sd.get('format') if isinstance(sd, dict) else type(sd).__name__!r})")
        if sd.get('version') != cls.STATE_VERSION:
            raise ValueError(f"from_state_dict: version {sd.get('version')!r} of the format is unknown (this library reads {cls.STATE_VERSION})")
        missing = [k for k in ('indptr', 'ts', 'nbr', 'eid', 'num_node', 't_last', 'time_ordered', 'strategy', 'seed', 'alpha',
                               'rng_kind', 'rng_key', 'rng_pos', 'rng_has_gauss', 'rng_cached_gaussian', 'mt_state') if k not in sd]
        if missing:
            raise ValueError(f'from_state_dict: the saved graph lacks {missing}')
        arrays = tuple(sd[k] for k in ('indptr', 'ts', 'nbr', 'eid'))
        if device is None:
            dev = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None
        else:
            dev = torch.device(device)
            dev = None if dev.type == 'cpu' else dev
        key, mt = sd['rng_key'], sd['mt_state']
        if verify:
            if not all(torch.is_tensor(a) for a in arrays):
                raise ValueError('from_state_dict: indptr, ts, nbr and eid must be tensors')
            n, _ = hip_ops._verify_arrays('from_state_dict', arrays, False)
            if isinstance(sd['num_node'], bool) or not isinstance(sd['num_node'], int) or sd['num_node'] != n:
                raise ValueError(f"from_state_dict: num_node = {sd['num_node']!r}, but indptr has {n} rows")
            if not isinstance(sd['strategy'], str) or not isinstance(sd['t_last'], float):
                raise ValueError('from_state_dict: strategy must be a str and t_last a float')
            if (not torch.is_tensor(key) or key.dtype != torch.int64 or tuple(key.shape) != (624,) or int(key.min()) < 0
                    or int(key.max()) > 0xFFFFFFFF or sd['rng_kind'] != 'MT19937' or not 0 <= int(sd['rng_pos']) <= 624):
                raise ValueError('from_state_dict: the saved rng state is no MT19937 state')
            if mt is not None and (not torch.is_tensor(mt) or mt.dtype != torch.int32 or tuple(mt.shape) != (625,)
                                   or not 0 <= int(mt[624]) <= 624):
                raise ValueError('from_state_dict: the saved device MT19937 state is no int32 [625] state')
        rng = np.random.RandomState()
        rng.set_state((str(sd['rng_kind']), key.numpy().astype(np.uint32), int(sd['rng_pos']), int(sd['rng_has_gauss']),
                       float(sd['rng_cached_gaussian'])))
        if dev is not None:
            with torch.cuda.device(dev):
                arrays = tuple(a.to(dev).contiguous() for a in arrays)
        else:
            arrays = tuple(np.array(a.numpy(), copy=True) for a in arrays)
        if verify:  # the arrays go nowhere else before this
            code, first, t_max = (hip_ops.tcsr_verify if dev is not None else hip_ops.tcsr_verify_host)(arrays, eid_rows)
            if code:
                raise ValueError('from_state_dict: ' + hip_ops.TCSR_VERIFY_TEXT(code, first))
            if not sd['t_last'] >= t_max:
                raise ValueError(f"from_state_dict: the saved latest time {sd['t_last']} is below the largest time of the "
                                 f'entries ({t_max})')
        self = cls.__new__(cls)
        self._init_common(int(sd['num_node']), sd['strategy'], sd['seed'], sd['alpha'], dev, rng=rng)
        self._time_ordered, self._t_last = bool(sd['time_ordered']), float(sd['t_last'])
        if dev is not None:
            self._adopt_device(arrays)
            if mt is not None:
                self._mt = mt.to(dev).contiguous()
        else:
            self._host = arrays
            if mt is not None:
                self._mt_saved = mt.clone()  # uploaded by `_mt_state` on first use
        return self

    # ---- online ingestion -----------------------------------------------------------
    def _num_node_arg(self, what: str, num_node):
        """the num_node argument of `extended` / `merged` -> (is it 'auto', the count an int asks for - else this graph's)"""
        auto = isinstance(num_node, str)
        if auto and num_node != 'auto':
            raise ValueError(f"{what}: num_node must be None, an int or 'auto', not {num_node!r}")
        n_out = self.num_node
        if num_node is not None and not auto:
            n_out = operator.index(num_node)
            if n_out < self.num_node:
                raise ValueError(f'{what}: num_node = {n_out} is below the graph\'s {self.num_node} (node ids are never released)')
            if n_out > 0x7FFFFFFF:
                raise ValueError(f'{what}: node ids must fit in 31 bits')
        return auto, n_out

    @staticmethod
    def _batch_arrays(what: str, src, dst, ts, eids):
        """a batch as given -> (on the device?, four flat contiguous int64 / int64 / float64 / int64 arrays - tensors on the
        device of a device `src`, numpy arrays otherwise -, the number of events)"""
        on_dev = torch.is_tensor(src) and src.device.type != 'cpu'
        if on_dev:
            batch = tuple(torch.as_tensor(x).to(src.device, dt).contiguous().reshape(-1)
                          for x, dt in zip((src, dst, ts, eids), (torch.int64, torch.int64, torch.float64, torch.int64)))
        else:
            np_of = lambda x, dt: np.ascontiguousarray(x.detach().numpy() if torch.is_tensor(x) else x, dtype=dt).reshape(-1)
            batch = (np_of(src, np.int64), np_of(dst, np.int64), np_of(ts, np.float64), np_of(eids, np.int64))
        n = int(batch[0].shape[0])
        if any(int(b.shape[0]) != n for b in batch):
            raise ValueError(f'{what}: src, dst, ts and eids must have one entry per event')
        return on_dev, batch, n

    def extended(self, src, dst, ts, eids, *, validate: bool = True, eid_rows: Optional[int] = None, num_node=None) -> 'Graph':
        """A NEW Graph over this graph's events followed by the batch (src, dst, ts, eids) - what `from_arrays` over the
        concatenated stream builds, bit for bit (tg_tcsr_append; graph.py:11-42,226-241 has no counterpart: the reference
        builds over the whole stream in advance).  This graph stays valid and unchanged: whatever holds it (captured
        graphs, resident evaluation runs, a collator thread) keeps working.  The batch must be non-decreasing in time and
        start no earlier than this graph's latest event (equal is allowed); ids in [0, num_node) - without the num_node
        argument below num_node does not grow, the model's tables are sized by it -; eids within 31 bits: ValueError
        otherwise, before anything is launched.
        Host inputs (numpy, CPU tensors) are checked on the host; device tensors with torch reductions and one read-back,
        or not at all with validate=False.  A device-resident parent costs no host work proportional to its size and no
        synchronisation (one launch pair over the old entries, on the current stream); the host view of the new graph is
        produced on first use.  strategy / seed / alpha / device carry over, and the child shares the parent's `rng` and
        device MT19937 state: 'uniform' draws continue one stream.  eid_rows: the rows of the caller's edge-feature table -
        an eid at or beyond it is refused with the rest (TIGE.observe; it shares the one read-back).
        num_node: admit new node ids (tg_tcsr_append_grow).  An int >= self.num_node: the child covers that
        many ids and the batch may name any id below it; 'auto': max(self.num_node, largest id of the batch + 1), from the
        maximum the validation reads back anyway (so refused with validate=False on a device batch; an explicit int is
        trusted there).  The child is what `from_arrays(..., max_node_id=num_node - 1)` over the concatenated stream
        builds, bit for bit; `trimmed`, `renumbered` and later `extended` calls keep its num_node.  The default None keeps
        num_node and refuses an id at or beyond it.  ValueError: an int below self.num_node or above 2^31 - 1."""
        auto, n_out = self._num_node_arg('extended', num_node)
        on_dev, batch, n = self._batch_arrays('extended', src, dst, ts, eids)
        if auto and n and on_dev and not validate:
            raise ValueError("extended: num_node='auto' takes the largest id from the validation's read-back; with "
                             'validate=False pass an int')
        t_last = self._t_last
        if n and (validate or not on_dev):
            if torch.is_tensor(t_last):
                t_last = self._t_last = float(t_last)
            s, d, t, e = batch
            if on_dev:  # a handful of reductions and the one read-back (ids and eids are exact in float64 below 2^53)
                ordered = (t[1:] >= t[:-1]).all().reshape(1)
                ints = torch.stack(torch.aminmax(torch.cat([s, d])) + torch.aminmax(e))
                st = torch.cat([ordered.double(), t[:1], t[-1:], ints.double()]).tolist()
            else:
                st = [float(n < 2 or np.all(t[1:] >= t[:-1])), t[0], t[-1], min(s.min(), d.min()), max(s.max(), d.max()),
                      e.min(), e.max()]
            if not st[0] or st[1] != st[1] or st[2] != st[2]:
                raise ValueError('extended: the batch must be non-decreasing in time')
            if st[1] < t_last:
                raise ValueError(f'extended: the batch starts at t = {st[1]}, before the latest event of the graph ({t_last})')
            if auto:
                if st[4] > 0x7FFFFFFE:
                    raise ValueError('extended: node ids must fit in 31 bits')
                n_out = max(self.num_node, int(st[4]) + 1)
            if st[3] < 0 or st[4] >= n_out:
                if num_node is not None:
                    raise ValueError(f'node ids must lie in [0, num_node) (num_node = {n_out})')
                raise ValueError('node ids must lie in [0, num_node) (num_node does not grow: the model\'s tables are sized by it)')
            if st[5] < 0 or st[6] > 0x7FFFFFFF:
                raise ValueError('edge ids must fit in 31 bits')
            if eid_rows is not None and st[6] >= eid_rows:
                raise ValueError(f'edge id {int(st[6])} is no row of the edge table ({eid_rows} rows)')
            t_last = float(st[2])
        elif n:
            t_last = batch[2][-1]  # trusted device batch: stays on the device until a later validation asks for it
        old_entries = self._dev[1].numel() if self._dev is not None else None
        if old_entries is None:
            self._materialise()
            if self._root.events is None:
                self._host_tcsr()
            old_entries = len(self._host[1]) if self._host is not None else 2 * len(self._root.events[0])
        if old_entries + 2 * n >= 2 ** 32:
            raise ValueError('extended: the device T-CSR holds fewer than 2^32 entries')
        child = self._child(n_out)
        child._t_last = t_last
        if self._dev is not None:  # device-resident parent: extend on the device
            dev = self._dev[0].device
            g = self.tcsr
            d_batch = batch if on_dev and batch[0].device == dev else tuple(torch.as_tensor(b).to(dev) for b in batch)
            batch = d_batch  # kept as uploaded (`last_batch`); the host view downloads it if it is ever asked for
            P = old_entries + 2 * n
            out = tcsr_arrays(n_out, P, dev)
            nbytes = int(lib.tg_tcsr_append_grow_workspace_bytes(old_entries, n, self.num_node, n_out))
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            # (inputs and workspace come from the caching allocator: their memory is reused in stream order, no wait needed)
            with torch.cuda.device(dev):
                check(lib.tg_tcsr_append_grow(C.byref(g), n_out, n, *(ptr(b) for b in d_batch), *(ptr(t) for t in out),
                                              ptr(ws), nbytes, stream_ptr(dev)), 'tg_tcsr_append')
            child._dev = out
            child._set_struct()
            child._mt = self._mt_state()
        child._root, child._log = self._root, (self._log, batch)
        child.last_batch = batch
        return child

    def widened(self, num_node: int) -> 'Graph':
        """`extended` with no events: a NEW Graph over the same entries that covers num_node >= self.num_node ids (the new
        ones own empty rows).  This graph stays valid and unchanged."""
        e = np.empty(0, dtype=np.int64)
        return self.extended(e, e, np.empty(0, dtype=np.float64), e, num_node=operator.index(num_node))

    # ---- late events ------------------------------------------------------------------
    def merged(self, src, dst, ts, eids, *, validate: bool = True, eid_rows: Optional[int] = None, num_node=None) -> 'Graph':
        """A NEW Graph over this graph's entries and the batch (src, dst, ts, eids), which may be in ANY order and hold ANY
        non-NaN times - before, inside or after this graph's range (tg_tcsr_merge; graph.py:11-42,226-241 has no
        counterpart: the reference sorts its lists once, over the whole stream).  Every row is the stable merge of the old
        row with the node's new entries sorted stably by time: at equal times the old entries first, then the new ones in
        event order (seen from src before seen from dst) - what `from_arrays` over [this graph's events | batch] builds, bit
        for bit, when this graph is the T-CSR of an event list, and the row-wise definition when it is not (a trimmed,
        erased or compacted parent).  A batch `extended` accepts gives the arrays `extended` gives.
        This graph stays valid and unchanged, and the child holds no reference to it: it adopts its arrays as a root of
        its own, as the children of `trimmed` / `without` do.  Inputs, validate, eid_rows and num_node (None / int / 'auto')
        are those of `extended`; a device-resident parent is merged on the device, on the current stream with
        allocator-owned buffers and no synchronisation beyond the validation's one read-back; a host-only parent takes the
        host twin.  strategy / seed / alpha / device carry over, the child shares `rng` and the device MT19937 state, has
        a `serial` of its own, and its latest event time is max(this graph's, the batch's).  On the host path with a known
        event list `_events` is the concatenation, and the time-ordered flag survives only if the concatenation really is
        ordered (the device builder's contract); on the device path `_events` is None and the flag is cleared.
        ValueError before anything is launched: a NaN time, ids outside [0, num_node), eids beyond 31 bits or beyond
        eid_rows, arrays of unequal length, 2^32 entries or more.  NOT refused: disorder, going back in time."""
        from ..hip_ops import tcsr_merge, tcsr_merge_host
        auto, n_out = self._num_node_arg('merged', num_node)
        on_dev, batch, n = self._batch_arrays('merged', src, dst, ts, eids)
        if auto and n and on_dev and not validate:
            raise ValueError("merged: num_node='auto' takes the largest id from the validation's read-back; with "
                             'validate=False pass an int')
        t_last = self._t_last
        if n and (validate or not on_dev):
            if torch.is_tensor(t_last):
                t_last = self._t_last = float(t_last)
            s, d, t, e = batch
            if on_dev:  # a handful of reductions and the one read-back (ids and eids are exact in float64 below 2^53)
                ints = torch.stack(torch.aminmax(torch.cat([s, d])) + torch.aminmax(e))
                st = torch.cat([(t != t).any().reshape(1).double(), t.max().reshape(1), ints.double()]).tolist()
            else:
                st = [float(np.isnan(t).any()), t.max(), min(s.min(), d.min()), max(s.max(), d.max()), e.min(), e.max()]
            if st[0]:
                raise ValueError('merged: a NaN time has no place in a row')
            if auto:
                if st[3] > 0x7FFFFFFE:
                    raise ValueError('merged: node ids must fit in 31 bits')
                n_out = max(self.num_node, int(st[3]) + 1)
            if st[2] < 0 or st[3] >= n_out:
                if num_node is not None:
                    raise ValueError(f'node ids must lie in [0, num_node) (num_node = {n_out})')
                raise ValueError('node ids must lie in [0, num_node) (num_node does not grow: the model\'s tables are sized by it)')
            if st[4] < 0 or st[5] > 0x7FFFFFFF:
                raise ValueError('edge ids must fit in 31 bits')
            if eid_rows is not None and st[5] >= eid_rows:
                raise ValueError(f'edge id {int(st[5])} is no row of the edge table ({eid_rows} rows)')
            t_last = max(t_last, float(st[1]))
        elif n:  # trusted device batch: the latest time stays on the device until a validation asks for it
            t_last = torch.maximum(torch.as_tensor(t_last, dtype=torch.float64, device=batch[2].device), batch[2].max())
        if self._dev is not None:
            old_entries = self._dev[1].numel()
        else:
            old_entries = len(self._host_tcsr()[1])
        if old_entries + 2 * n >= 2 ** 32:
            raise ValueError('merged: the device T-CSR holds fewer than 2^32 entries')
        child = self._child(n_out)
        child._t_last = t_last
        if self._dev is not None:  # device-resident parent: merge on the device
            dev = self._dev[0].device
            d_batch = batch if on_dev and batch[0].device == dev else tuple(torch.as_tensor(b).to(dev) for b in batch)
            child._time_ordered = self._time_ordered and n == 0
            return child._adopt_device(tcsr_merge(self, d_batch, n_out), self)
        if on_dev:
            batch = tuple(np.ascontiguousarray(b.cpu().numpy()) for b in batch)
        out = tcsr_merge_host(self, batch, n_out)
        ev = self._root.events
        if ev is not None:
            ev = tuple(np.concatenate([a, b]) for a, b in zip(ev, batch))
            child._time_ordered = bool(self._time_ordered and np.all(ev[2][1:] >= ev[2][:-1]))
        else:
            child._time_ordered = self._time_ordered and n == 0
        return child._adopt_host(out, ev, self)

    # ---- sliding-window expiry --------------------------------------------------------
    def trimmed(self, before: Optional[float] = None, keep_last: Optional[int] = None) -> 'Graph':
        """A NEW Graph without this graph's expired entries (tg_tcsr_trim_*; graph.py:11-42 has no counterpart: the
        reference builds its adjacency lists once and never drops an entry).  An entry is dropped if its time is strictly
        below `before` (the float64 '<' of every sampler's cut) or if it is not among its node's last `keep_last` entries;
        None switches a rule off, both None give a copy.  This graph stays valid and unchanged, and the child holds no
        reference to it: dropping the parent releases its memory.  num_node does not change.
        A device-resident parent is trimmed on the device, on the current stream with allocator-owned buffers: a plan
        over the nodes, ONE int64 read back (the number of kept entries - the only synchronisation - so that the child's
        arrays are allocated exactly), a copy over the kept entries.  A host-only parent takes the host twin at once.
        strategy / seed / alpha / device carry over, the child shares the parent's `rng` and device MT19937 state, and it
        keeps the parent's latest event time EVEN WHEN EVERY ENTRY WAS DROPPED: a later `extended` still refuses to go
        back in time.  The child has a `serial` of its own.  Its host view is produced on first use (downloaded from its
        own device arrays); a graph trimmed on the device, or with a cap, no longer corresponds to an event list and has
        `_events` None.  `extended`, `to` and the samplers work on it as on any graph.
        Guarantees: with `before` alone the result is what `from_arrays` over the events with ts >= before builds, bit
        for bit.  After any trim a query (v, t) sees the parent's entries before t restricted to the kept ones, so
        `recent_edges` with K <= keep_last and `get_history` with H <= keep_last return the parent's result at every t
        later than the graph's latest time.  (A second hop is sampled at the neighbours' EARLIER times: no such guarantee.)
        ValueError before anything is launched: a NaN `before`, a negative `keep_last`."""
        t_cut = -np.inf if before is None else float(before)
        if t_cut != t_cut:
            raise ValueError('trimmed: `before` is NaN')
        keep = -1 if keep_last is None else operator.index(keep_last)
        if keep_last is not None and keep < 0:
            raise ValueError(f'trimmed: keep_last = {keep} is negative')
        child = self._child()
        if self._dev is not None:  # device-resident parent: plan, one read-back, allocate exactly, apply
            plan = ('tg_tcsr_trim_plan', lambda g, *out: lib.tg_tcsr_trim_plan(g, t_cut, keep, *out))
            return child._adopt_device(tcsr_compacted(self, lambda g: lib.tg_tcsr_trim_workspace_bytes(g.num_node), plan,
                                                      ('tg_tcsr_trim_apply', lib.tg_tcsr_trim_apply)), self)
        out = tcsr_compacted_host(self, 'tg_tcsr_trim_host', lambda g, *out: lib.tg_tcsr_trim_host(g, t_cut, keep, *out))
        ev = self._root.events if keep_last is None else None  # a horizon alone: still the T-CSR of an event list
        if ev is not None:
            m = ev[2] >= t_cut
            ev = tuple(np.ascontiguousarray(a[m]) for a in ev)
        return child._adopt_host(out, ev, self)

    # ---- erasing nodes, retracting events ----------------------------------------------
    @staticmethod
    def _erase_ids(what, ids):
        """an int sequence / tensor of ids -> (int64 array or tensor as given, flattened; min; max), None for None"""
        if ids is None:
            return None
        if torch.is_tensor(ids):
            if ids.numel() and (ids.dtype.is_floating_point or ids.dtype == torch.bool):
                raise ValueError(f'without: {what} are integer ids, not {ids.dtype}')
            ids = ids.detach().to(torch.int64).contiguous().reshape(-1)
            lo, hi = (int(x) for x in torch.aminmax(ids)) if ids.numel() else (0, -1)
        else:
            ids = np.asarray(ids)
            if ids.size and ids.dtype.kind not in 'iu':
                raise ValueError(f'without: {what} are integer ids, not {ids.dtype}')
            ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            lo, hi = (int(ids.min()), int(ids.max())) if ids.size else (0, -1)
        return ids, lo, hi

    def without(self, nodes=None, eids=None, *, eid_rows: Optional[int] = None) -> 'Graph':
        """A NEW Graph without the entries of the erased `nodes` and the retracted events `eids` (tg_tcsr_erase_*;
        graph.py:11-42 has no counterpart: the reference never takes a node or an event out).  An entry is dropped if its
        owner or its neighbour is one of `nodes`, or if its edge id is one of `eids` (both entries of an event name it and
        go together); every other entry stays, bit for bit and in order - what `from_arrays` over the events with src, dst
        not in `nodes` and eid not in `eids` builds (max_node_id = num_node - 1).  num_node does not change: an erased node
        owns an empty row, and a later `extended` may bring its id back as a node never seen.  nodes / eids: int sequences
        or tensors, duplicates are fine, an eid that names no entry is a no-op; the bitmaps are built with `new_bitmap` and
        `bitmap_mark`; eid_rows: the ids the eid bitmap covers (default 1 + max(eids); an eid at or beyond it is not
        retracted).
        This graph stays valid and unchanged, and the child holds no reference to it.  A device-resident parent is
        compacted on the device, on the current stream with allocator-owned buffers: a plan over tiles of the old entries,
        ONE int64 read back (the number of kept entries - the only synchronisation - so that the child's arrays are
        allocated exactly), a copy.  A host-only parent takes the host twin at once.  strategy / seed / alpha / device
        carry over, the child shares the parent's `rng` and device MT19937 state, keeps the parent's latest event time EVEN
        WHEN EVERY ENTRY WENT and the time-ordered flag, and has a `serial` of its own.  On the host path with a known
        event list `_events` is the filtered list; on the device path it is None.
        ValueError before anything is launched: a node id outside [0, num_node), node id 0 (the padding id can never be
        erased), a negative eid or one beyond 31 bits, both arguments None, an eid_rows that is negative."""
        from .. import hip_ops
        if nodes is None and eids is None:
            raise ValueError('without: pass nodes, eids or both (both None erases nothing)')
        nd, ed = self._erase_ids('nodes', nodes), self._erase_ids('eids', eids)
        if nd is not None and len(nd[0]):
            if nd[1] < 0 or nd[2] >= self.num_node:
                raise ValueError(f'without: node ids must lie in [0, num_node) (num_node = {self.num_node})')
            if nd[1] == 0:
                raise ValueError('without: node id 0 is the padding id and can never be erased')
        if ed is not None and len(ed[0]) and (ed[1] < 0 or ed[2] > 0x7FFFFFFF):
            raise ValueError('without: edge ids are non-negative and fit in 31 bits')
        if eid_rows is None:
            n_rows = ed[2] + 1 if ed is not None and len(ed[0]) else 0
        else:
            n_rows = operator.index(eid_rows)
            if n_rows < 0 or n_rows > 0x80000000:
                raise ValueError(f'without: eid_rows = {n_rows} is outside [0, 2^31]')
        child = self._child()
        if self._dev is not None:  # device-resident parent: plan, one read-back, allocate exactly, apply
            dev = self._dev[0].device
            node_bits = eid_bits = None
            with torch.cuda.device(dev):
                if nd is not None:
                    node_bits = hip_ops.new_bitmap(self.num_node, dev)
                    hip_ops.bitmap_mark(torch.as_tensor(nd[0]).to(dev), node_bits, self.num_node)
                if ed is not None and n_rows > 0:
                    eid_bits = hip_ops.new_bitmap(n_rows, dev)
                    hip_ops.bitmap_mark(torch.as_tensor(ed[0]).to(dev), eid_bits, n_rows)  # (ids >= n_rows are not marked)
            indptr, P, ws = hip_ops.tcsr_erase_plan(self, node_bits, eid_bits, n_rows if eid_bits is not None else 0)
            return child._adopt_device((indptr,) + hip_ops.tcsr_erase_apply(self, indptr, P, ws), self)
        else:
            to_np = lambda x: x.cpu().numpy() if torch.is_tensor(x) else x
            n_ids = to_np(nd[0]) if nd is not None else None
            e_ids = to_np(ed[0]) if ed is not None else None
            node_bits = hip_ops.host_bitmap(n_ids, self.num_node) if nd is not None else None
            eid_bits = hip_ops.host_bitmap(e_ids, n_rows) if ed is not None and n_rows > 0 else None
            out = hip_ops.tcsr_erase_host(self, node_bits, eid_bits, n_rows if eid_bits is not None else 0)
            ev = self._root.events
            if ev is not None:  # still the T-CSR of an event list: the filtered one
                m = np.ones(len(ev[0]), dtype=bool)
                if nd is not None:
                    m &= ~np.isin(ev[0], n_ids) & ~np.isin(ev[1], n_ids)
                if eid_bits is not None:
                    m &= ~np.isin(ev[3], e_ids[e_ids < n_rows])
                ev = tuple(np.ascontiguousarray(a[m]) for a in ev)
            return child._adopt_host(out, ev, self)

    # ---- renumbered edge ids ---------------------------------------------------------
    def renumbered(self, remap, eid_out) -> 'Graph':
        """A NEW Graph whose entries name the rows of a packed edge table (tg_edge_rows_*: hip_ops.edge_rows_plan / _apply /
        _host; graph.py:11-42 has no counterpart: the reference never drops a table row).  `eid_out` is this graph's eid
        array pushed through `remap` (old row -> new row, -1: released), bit 31 - the direction flag - carried over.  The
        child SHARES indptr, ts and nbr with this graph (the same tensors / arrays) and owns `eid_out`; this graph stays
        valid and unchanged.  strategy / seed / alpha / device, `rng` and device MT19937 state, the latest event time and
        the time-ordered flag carry over; the child has a `serial` and a host origin of its own, as a trimmed child has.
        A device-resident parent keeps eid_out on its device, a host-only parent as a numpy array (either is moved there
        if it is not); the event list is pushed through `remap` on the host path and dropped on the device path
        (`_events` None).  ValueError: eid_out is no int32 array of num_entry entries."""
        child = self._child()
        if self._dev is not None:
            d = self._dev
            eid_out = torch.as_tensor(eid_out)
            if eid_out.dtype != torch.int32 or eid_out.dim() != 1 or eid_out.numel() != d[3].numel():
                raise ValueError(f'renumbered: eid_out must be an int32 array of {d[3].numel()} entries')
            eid_out = eid_out.to(d[3].device).contiguous()  # (a host twin's result for a device-resident graph is uploaded)
            return child._adopt_device((d[0], d[1], d[2], eid_out), self)
        else:
            h = self._host_tcsr()
            e = np.ascontiguousarray(eid_out.cpu().numpy() if torch.is_tensor(eid_out) else eid_out)
            if e.dtype != np.int32 or e.shape != h[3].shape:
                raise ValueError(f'renumbered: eid_out must be an int32 array of {len(h[3])} entries')
            ev, events = self._root.events, None
            if ev is not None and remap is not None:
                r = np.asarray(remap.cpu().numpy() if torch.is_tensor(remap) else remap)
                new = r[ev[3]].astype(np.int64) if len(ev[3]) == 0 or int(ev[3].max()) < len(r) else None
                if new is not None and (len(new) == 0 or new.min() >= 0):  # (every event's row survived: still an event list)
                    events = (ev[0], ev[1], ev[2], new)
            return child._adopt_host((h[0], h[1], h[2], e), events, self)

    # ---- compacted node ids ------------------------------------------------------------
    def compacted(self, plan) -> 'Graph':
        """A NEW Graph over the densely renumbered node ids of `plan` (tg_node_compact_*: hip_ops.node_compact_plan /
        node_compact_host OVER THIS GRAPH; graph.py:11-42 has no counterpart: the reference never releases a node id).  A
        dropped id owns no entry and is nobody's neighbour (the plan refuses anything else), so no entry moves: the child
        SHARES ts and eid with this graph (the same tensors / arrays) and owns plan.indptr - the bounds of the kept rows -
        and plan.nbr = remap[nbr]; num_node = plan.n_graph_new.  This graph stays valid and unchanged.  The result equals,
        bit for bit, `from_arrays` over this graph's events with src / dst passed through plan.remap
        (max_node_id = num_node - 1).  strategy / seed / alpha / device, `rng` and device MT19937 state, the latest event
        time and the time-ordered flag carry over; the child has a `serial` and a host origin of its own.  A
        device-resident parent takes a device plan, a host-only parent a plan of the host twin; the event list is pushed
        through remap on the host path and dropped on the device path (`_events` None).  ValueError: a plan with an error
        class, of another graph size, or on the other side (device / host)."""
        if plan.code:
            from ..hip_ops import NODE_COMPACT_TEXT
            raise ValueError('compacted: ' + NODE_COMPACT_TEXT(plan.code, plan.first, plan.n_old))
        if plan.indptr is None or plan.n_graph_old != self.num_node:
            raise ValueError(f'compacted: the plan covers a graph of {plan.n_graph_old if plan.indptr is not None else 0} '
                             f'nodes, this graph has {self.num_node}')
        child = self._child(plan.n_graph_new)
        if self._dev is not None:
            d = self._dev
            if not torch.is_tensor(plan.nbr) or plan.nbr.device != d[2].device or plan.nbr.numel() != d[2].numel():
                raise ValueError(f'compacted: a device-resident graph takes a plan of node_compact_plan over its '
                                 f'{d[2].numel()} entries on {d[2].device}')
            return child._adopt_device((plan.indptr, d[1], plan.nbr, d[3]), self)
        h = self._host_tcsr()
        if not isinstance(plan.nbr, np.ndarray) or plan.nbr.shape != h[2].shape:
            raise ValueError(f'compacted: a host graph takes a plan of node_compact_host over its {len(h[2])} entries')
        ev = self._root.events
        if ev is not None:
            r = plan.remap.numpy().astype(np.int64)
            ev = (r[ev[0]], r[ev[1]], ev[2], ev[3])
        return child._adopt_host((plan.indptr, h[1], plan.nbr, h[3]), ev, self)

    # ---- sampling -------------------------------------------------------------------
    def sample_device(self, nids: Tensor, ts: Tensor, n_neighbors: int, strategy: Optional[str] = None,
                      mark_flags: Optional[Tensor] = None, want_dirs: bool = True
                      ) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
        """Device-tensor form of sample_temporal_neighbor: nids int64[Q], ts float64[Q]."""
        strategy = self.strategy if strategy is None else strategy
        g = self.tcsr
        dev = self.device
        nids = nids.to(dev, torch.int64).contiguous()
        ts = ts.to(dev, torch.float64).contiguous()  # float32 queries widen exactly (np.searchsorted does the same)
        Q, K = nids.numel(), int(n_neighbors)
        assert ts.numel() == Q
        o_n = torch.empty(Q, K, dtype=torch.int64, device=dev)
        o_e = torch.empty(Q, K, dtype=torch.int64, device=dev)
        o_t = torch.empty(Q, K, dtype=torch.float32, device=dev)
        o_d = torch.empty(Q, K, dtype=torch.int64, device=dev) if want_dirs else None
        s = stream_ptr(dev)
        if strategy == 'recent_edges':
            check(lib.tg_sample_recent_edges(C.byref(g), Q, ptr(nids), ptr(ts), K, ptr(o_n), ptr(o_e), ptr(o_t),
                                             ptr(o_d), ptr(mark_flags), s), 'tg_sample_recent_edges')
        elif strategy == 'recent_nodes':
            check(lib.tg_sample_recent_nodes(C.byref(g), Q, ptr(nids), ptr(ts), K, ptr(o_n), ptr(o_e), ptr(o_t),
                                             ptr(o_d), s), 'tg_sample_recent_nodes')
        elif strategy == 'uniform':
            check(lib.tg_sample_uniform(C.byref(g), Q, ptr(nids), ptr(ts), K, ptr(self._mt_state()), ptr(o_n),
                                        ptr(o_e), ptr(o_t), ptr(o_d), s), 'tg_sample_uniform')
        else:
            raise NotImplementedError(strategy)
        if mark_flags is not None and strategy != 'recent_edges':
            from ..hip_ops import flags_mark
            flags_mark(nids, mark_flags, self.num_node)
            flags_mark(o_n.reshape(-1), mark_flags, self.num_node)
        return o_n, o_e, o_t, o_d

    def sample_temporal_neighbor(self, nids: np.ndarray, ts: np.ndarray, n_neighbors: int = 20,
                                 strategy: Optional[str] = None
                                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """graph.py:67-148 - numpy in, numpy out: ([bs,K] int64 neighbours, [bs,K] int64 edge ids,
        [bs,K] float32 timestamps, [bs,K] int64 directions), left padded with zeros."""
        assert len(nids) == len(ts)
        n_t = torch.from_numpy(np.ascontiguousarray(nids, dtype=np.int64))
        t_t = torch.from_numpy(np.ascontiguousarray(ts, dtype=np.float64))
        out = self.sample_device(n_t, t_t, n_neighbors, strategy)
        return tuple(o.cpu().numpy() for o in out)

    def get_history(self, nids: np.ndarray, ts: np.ndarray, hist_len: int):
        """graph.py:150-155"""
        return self.sample_temporal_neighbor(nids, ts, n_neighbors=hist_len, strategy='recent_edges')
