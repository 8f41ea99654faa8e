"""Numpy reference and shared inputs of the snapshot-refresh tests (tests/test_snapshot_refresh_host.py,
tests/test_hip_snapshot_refresh.py, tests/test_hip_refresh_model.py).  Row j of a catalogue is dirty iff
touched[numpy_involved(og, [ids[j]], [t_row[j]], K, L, strategy)].any() or its age exceeds max_age (strict float64);
rank / cols follow from the flags; the merge is a np.where over the row tables; the degree difference compares np.diff of
two indptr arrays.  The involved set of a (node, time) query does not depend on the bitmap, so it is computed once per
(graph, strategy, K, layers, node, time) and shared."""
import numpy as np

import _involved_ref as R

GRAPH_NAMES = ('stream76', 'hand64', 'hand65', 'hand129')
_INV = {}
_OG = {}


def oracle_graph(name, strategy):
    if (name, strategy) not in _OG:
        _OG[name, strategy] = R.oracle_graph(R.events(name), strategy)
    return _OG[name, strategy]


def oracle_from_arrays(indptr, ts, nbr, eid, strategy):
    """the oracle's graph (its samplers, its strict cut) over given T-CSR arrays instead of an event list - for graphs that
    no event list describes (trimmed per node, entries erased)"""
    from oracle import tiger_oracle as O
    og = O.OracleGraph.__new__(O.OracleGraph)
    og.indptr = np.asarray(indptr, np.int64)
    og.ts, og.nbr = np.asarray(ts, np.float64), np.asarray(nbr, np.int64)
    og.eid = np.asarray(eid, np.int64) & 0x7fffffff
    og.dir = np.zeros(len(og.ts), np.int64)
    og.num_node, og.strategy, og.rng = len(og.indptr) - 1, strategy, np.random.RandomState(0)
    return og


def involved_of(name, strategy, K, L, nid, t, og=None):
    """numpy_involved of the one query (nid, t); `og`: an oracle graph that is not one of the named ones (then `name` is any
    key that tells it apart)"""
    key = (name, strategy, K, L, int(nid), float(t))
    if key not in _INV:
        og = oracle_graph(name, strategy) if og is None else og
        _INV[key] = R.numpy_involved(og, [int(nid)], [float(t)], K, L, strategy)
    return _INV[key]


def catalogue(ev, C, uniform_time=False):
    """C catalogue rows (id, time): the query list of _involved_ref.queries - its edge cases in front (the float32 case, the
    padding id 0, the last node, a node before its first event, a time equal to an event's, a row twice) - repeated to C
    rows, so ids repeat.  uniform_time: every row at one time after the last event (-> ids, that time)."""
    pool_n, pool_t = R.queries(ev, 192)
    idx = np.arange(C) % 192
    ids = pool_n[idx].astype(np.int64)
    if uniform_time:
        return ids, float(ev['ts'].max()) + 1.0
    return ids, pool_t[idx].astype(np.float64)


def touched_states(n_nodes, seed=0):
    """empty, full, a random half, single bits at ids 63, 64 and n - 1 (where the graph has them)"""
    st = dict(R.uptodate_states(n_nodes, seed + 5))
    for v in (63, 64, n_nodes - 1):
        if v < n_nodes:
            one = np.zeros(n_nodes, bool)
            one[v] = True
            st[f'bit{v}'] = one
    return st


def dirty(name, strategy, K, L, ids, t_row, touched, t_new, max_age=None, og=None):
    """-> dict(touched bool [C], aged bool [C], rank int32 [C], cols int32 [n], count (n_dirty, n_by_age_alone));
    t_row: an array or one float"""
    ids = np.asarray(ids, np.int64)
    C = len(ids)
    t_row = np.full(C, t_row, np.float64) if np.isscalar(t_row) else np.asarray(t_row, np.float64)
    hit = np.array([touched[involved_of(name, strategy, K, L, v, t, og)].any() for v, t in zip(ids, t_row)], bool).reshape(C)
    aged = np.zeros(C, bool) if max_age is None else (np.float64(t_new) - t_row) > np.float64(max_age)
    flag = hit | aged
    cols = np.nonzero(flag)[0].astype(np.int32)
    rank = np.where(flag, np.cumsum(flag) - 1, -1).astype(np.int32)
    return dict(touched=hit, aged=aged, rank=rank, cols=cols, count=(int(flag.sum()), int((aged & ~hit).sum())))


def merge(rank, old, new):
    """out[j] = new[rank[j]] where rank[j] >= 0 else old[j]; old [C, ...], new [n, ...] (n may be 0)"""
    rank = np.asarray(rank)
    if len(new) == 0:
        return old.copy()
    pick = new[np.clip(rank, 0, len(new) - 1)]
    sel = (rank >= 0).reshape((-1,) + (1,) * (old.ndim - 1))
    return np.where(sel, pick, old)


def merge_times(rank, t_old, t_new):
    rank = np.asarray(rank)
    t_old = np.full(len(rank), t_old, np.float64) if np.isscalar(t_old) else np.asarray(t_old, np.float64)
    return np.where(rank >= 0, np.float64(t_new), t_old)


def degree_diff(indptr_a, indptr_b):
    """bool [max(n_a, n_b)]: the row lengths differ, an id beyond a graph's node count has length 0 there"""
    la, lb = np.diff(np.asarray(indptr_a)), np.diff(np.asarray(indptr_b))
    n = max(len(la), len(lb))
    la, lb = np.pad(la, (0, n - len(la))), np.pad(lb, (0, n - len(lb)))
    return la != lb
