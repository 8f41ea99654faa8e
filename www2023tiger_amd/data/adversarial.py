"""Historical and inductive negative sampling for link evaluation.

Mirror of tiger/data/adversarial.py (`AdversarialEdgeSampler`, the `hist` / `ind` negatives of Poursafaei et al.,
NeurIPS 2022): same constructor, attributes, methods, return types and errors.  The reference rebuilds the edge sets
of the whole stream up to each chunk's time in a Python loop; here every query is one wavefront filtering the
source's time-sorted T-CSR entries before t0 against a pair index built once (csrc/tg_adv.hip), and
`pre_sample_neg_dsts` is one launch for all chunks.  Without a GPU the library's host twins compute the same values.

Declared difference: the random stream is not numpy's.  The reference draws `rng.choice(list(set))`, which depends on
CPython's set iteration order; here the candidates are taken in T-CSR order and indexed by a counter-based hash
(tiger_hip.h: tg_adv_neg_sample).  Candidate sets, the uniform fallback over `full_dst_distinct` and the uniform
distribution over each set are the reference's.
"""
import ctypes as C
import os
from collections import defaultdict
from typing import Dict, Optional, Set

import numpy as np
import torch

from .._lib import TG_ADV_HIST, TG_ADV_IND, TgAdvIndex, check, lib, ptr
from ..hip_ops import stream_ptr
from .graph import Graph

_MODES = {'hist': TG_ADV_HIST, 'ind': TG_ADV_IND}


class AdversarialEdgeSampler:
    """Adversarial random edge sampling as negative edges (adversarial.py:8-117)."""

    def __init__(self, full_srcs, full_dsts, full_ts, test_srcs, test_ts, neg_type, seed=None, *,
                 graph: Optional[Graph] = None, device=None):
        """`full_*` is the whole stream (train, validation and test events), time-ordered; `test_*` is its tail.
        graph: an existing `Graph` over the same full stream whose T-CSR is reused.  device: where the queries run
        (default: the graph's device, else cuda:0 when a GPU is visible; 'cpu' or no GPU: the host twins)."""
        if not (neg_type == 'hist' or neg_type == 'ind'):
            raise ValueError("Undefined Negative Edge Sampling Strategy!")
        self.seed = seed
        self.neg_type = neg_type
        self.full_srcs = full_srcs
        self.full_dsts = full_dsts
        self.full_ts = full_ts
        ts = np.asarray(full_ts, dtype=np.float64)
        if len(ts) > 1 and np.any(ts[1:] < ts[:-1]):
            raise ValueError('full_ts must be sorted in time (the time windows are found by binary search)')
        self.full_srcs_distinct = np.unique(full_srcs)
        self.full_dst_distinct = np.unique(full_dsts)
        self.full_ts_distinct = np.unique(full_ts)
        self.test_srcs = test_srcs
        self.test_ts = test_ts
        self.ts_init = min(self.full_ts_distinct)
        self.ts_end = max(self.full_ts_distinct)
        self.ts_hist_end = self.full_ts[-len(test_srcs) - 1]
        self._train_edge_dict = None
        if device is None:
            if graph is not None and graph._device is not None:
                device = graph._device
            elif torch.cuda.is_available():
                device = torch.device('cuda', 0)
        self._device = torch.device(device) if device is not None else None
        if self._device is not None and self._device.type == 'cpu':
            self._device = None
        if graph is None:
            src = np.ascontiguousarray(full_srcs, dtype=np.int64)
            dst = np.ascontiguousarray(full_dsts, dtype=np.int64)
            graph = Graph.from_arrays(src, dst, ts, np.arange(len(src), dtype=np.int64), strategy='recent_edges',
                                      device=self._device)
        elif self._device is not None:
            graph.to(self._device)
        self.graph = graph
        self._ix = None  # (next_ts, first_ts) aligned with the T-CSR, on the device or the host
        self._dd = None  # full_dst_distinct as int64 where the queries run
        self.reset_random_state()

    # ---- the reference's set-based helpers (kept for API parity; the sampler does not use them) ---------------------
    @property
    def train_edge_dict(self) -> Dict[int, Set[int]]:
        """edges up to ts_hist_end (adversarial.py:34), built on first use"""
        if self._train_edge_dict is None:
            self._train_edge_dict = self.get_edges_within(self.ts_init, self.ts_hist_end)
        return self._train_edge_dict

    @train_edge_dict.setter
    def train_edge_dict(self, value):
        self._train_edge_dict = value

    def get_edges_within(self, t0: float, t1: float, subset: Optional[Set] = None) -> Dict[int, Set[int]]:
        """{src: set of dst} over the events with t0 <= ts <= t1 (by binary search on full_ts)"""
        lo = np.searchsorted(self.full_ts, t0, side='left')
        hi = np.searchsorted(self.full_ts, t1, side='right')
        out = defaultdict(set)
        keep = None if subset is None else set(np.asarray(list(subset)).tolist())
        for s, d in zip(self.full_srcs[lo:hi], self.full_dsts[lo:hi]):
            if keep is None or s in keep:
                out[s].add(d)
        return out

    def get_difference_edge_list(self, first_e_set, second_e_set):
        """(srcs, dsts) of the (src, dst) pairs in the first set and not in the second"""
        diff = set(first_e_set) - set(second_e_set)
        return np.array([e[0] for e in diff]), np.array([e[1] for e in diff])

    # ---- sampling --------------------------------------------------------------------------------------------------
    def reset_random_state(self):
        """back to the first draw of the seed's stream (seed None: a fresh seed from OS entropy)"""
        self._seed = int(self.seed) & (2 ** 64 - 1) if self.seed is not None else int.from_bytes(os.urandom(8), 'little')
        self._counter = 0

    def sample(self, srcs, t0, t1):
        if self.neg_type == 'hist':
            neg_srcs, neg_dsts = self.sample_hist(srcs, t0, t1)
        elif self.neg_type == 'ind':
            neg_srcs, neg_dsts = self.sample_ind(srcs, t0, t1)
        else:
            raise ValueError("Undefined Negative Edge Sampling Strategy!")
        return neg_srcs, neg_dsts

    def sample_hist(self, srcs, t0, t1):
        return srcs, self._draw('hist', srcs, t0, t1)

    def sample_ind(self, srcs, t0, t1):
        return srcs, self._draw('ind', srcs, t0, t1)

    def pre_sample_neg_dsts(self, n_total: int, bs: int = 200) -> np.ndarray:
        """one negative per test event, chunk i of `bs` events queried in [ts of its first, ts of its last event]
        (adversarial.py:105-117) - all chunks in one launch; every call returns the same array"""
        self.reset_random_state()
        assert len(self.test_srcs) == n_total
        test_ts = np.asarray(self.test_ts, dtype=np.float64)
        first = (np.arange(n_total) // bs) * bs
        last = np.minimum(first + bs, n_total) - 1
        out = self._draw(self.neg_type, self.test_srcs, test_ts[first], test_ts[last])
        assert len(out) == n_total
        return out

    def _draw(self, neg_type, srcs, t0, t1) -> np.ndarray:
        """one launch over len(srcs) queries with per-query (or scalar) windows; advances the counter"""
        srcs = np.ascontiguousarray(srcs, dtype=np.int64).reshape(-1)
        n = len(srcs)
        t0 = np.array(np.broadcast_to(np.asarray(t0, dtype=np.float64), (n,)))
        t1 = np.array(np.broadcast_to(np.asarray(t1, dtype=np.float64), (n,)))
        if np.any(~(t0 <= t1)):
            raise ValueError('t0 must not be later than t1')
        out = self._launch(_MODES[neg_type], srcs, t0, t1, self._counter)
        self._counter += 1
        return out

    def _index(self):
        g = self.graph
        if self._ix is not None and self._ix_serial != g.serial:
            self._ix = None  # `graph` was replaced (Graph.extended): the index is aligned with the arrays of the graph it saw
        if self._ix is None:
            if self._device is None:
                h = g._host_tcsr()
                self._tcsr_h = _host_struct(g.num_node, h)
                P = len(h[1])
                nxt, fst = np.empty(P, dtype=np.float64), np.empty(P, dtype=np.float64)
                check(lib.tg_adv_index_build_host(C.byref(self._tcsr_h), ptr(nxt), ptr(fst)), 'tg_adv_index_build_host')
                self._dd = np.ascontiguousarray(self.full_dst_distinct, dtype=np.int64)
            else:
                dev = self._device
                tc = g.tcsr
                P = int(tc.num_entry)
                nxt = torch.empty(P, dtype=torch.float64, device=dev)
                fst = torch.empty(P, dtype=torch.float64, device=dev)
                nbytes = int(lib.tg_adv_index_build_device_workspace_bytes(P, g.num_node))
                ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
                check(lib.tg_adv_index_build_device(C.byref(tc), ptr(nxt), ptr(fst), ptr(ws), nbytes, stream_ptr(dev)),
                      'tg_adv_index_build_device')
                torch.cuda.current_stream(dev).synchronize()  # the workspace dies with this scope
                self._dd = torch.from_numpy(np.ascontiguousarray(self.full_dst_distinct, dtype=np.int64)).to(dev)
            if P != 2 * len(self.full_srcs):
                raise ValueError('the graph is not over the full stream (it needs two T-CSR entries per event)')
            self._ix = (nxt, fst)
            self._ix_serial = g.serial
        return self._ix

    def _launch(self, mode, srcs, t0, t1, counter, out_count=False):
        nxt, fst = self._index()
        ix = TgAdvIndex(ptr(nxt), ptr(fst))
        n = len(srcs)
        seed = C.c_uint64(self._seed)
        if self._device is None:
            out = np.empty(n, dtype=np.int64)
            cnt = np.empty(n, dtype=np.int64) if out_count else None
            check(lib.tg_adv_neg_sample_host(C.byref(self._tcsr_h), C.byref(ix), n, ptr(srcs), ptr(t0), ptr(t1), mode,
                                             float(self.ts_hist_end), ptr(self._dd), len(self._dd), seed, counter,
                                             ptr(out), ptr(cnt)), 'tg_adv_neg_sample_host')
            return (out, cnt) if out_count else out
        dev = self._device
        d_srcs, d_t0, d_t1 = (torch.from_numpy(a).to(dev) for a in (srcs, t0, t1))
        out = torch.empty(n, dtype=torch.int64, device=dev)
        cnt = torch.empty(n, dtype=torch.int64, device=dev) if out_count else None
        check(lib.tg_adv_neg_sample(C.byref(self.graph.tcsr), C.byref(ix), n, ptr(d_srcs), ptr(d_t0), ptr(d_t1), mode,
                                    float(self.ts_hist_end), ptr(self._dd), len(self._dd), seed, counter, ptr(out),
                                    ptr(cnt), stream_ptr(dev)), 'tg_adv_neg_sample')
        out = out.cpu().numpy()
        return (out, cnt.cpu().numpy()) if out_count else out


def _host_struct(num_node, h):
    from .._lib import TgTcsr
    indptr, ts, nbr, eid = h
    return TgTcsr(num_node, len(ts), ptr(indptr), ptr(ts), ptr(nbr), ptr(eid))
