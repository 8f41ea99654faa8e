"""Reference, caps and cases of the walk-candidate tests (tests/test_walk_host.py, tests/test_hip_walk.py).

The reference is written from the contract of tg_walk_candidates (include/tiger_hip.h) and shares nothing with the library:
per-node time-sorted entries from one np.lexsort, np.searchsorted(side='left') for the strict cut, a dict for the weights
and sorted(key=(-w, id)) for the order.  Everything is integer work: every comparison in the tests is exact."""
import numpy as np

import _cap_ref

# ---- the caps (include/tiger_hip.h) and the grid cap of the launch, with the source line it mirrors -----------------------
MAX_FANOUT = 64        # `#define TG_WALK_MAX_FANOUT 64`
MAX_FRONTIER = 1024    # `#define TG_WALK_MAX_FRONTIER 1024`
MAX_ENDPOINTS = 2048   # `#define TG_WALK_MAX_ENDPOINTS 2048`
# tg_walk.hip: tg_walk_candidates: `dim3(flat_grid(B, 1))` - one workgroup per query, flat_grid caps the blocks
PER_WORKGROUP = 1
CAP_WALK = _cap_ref.FLAT_BLOCKS * PER_WORKGROUP            # 4 096 queries: the last size without a second pass
Q_WALK_AT, Q_WALK_PAST = CAP_WALK, _cap_ref.past(CAP_WALK, 5)

DEFAULT = ((10, 10, 10), (True, False, True))
# (fanout, take): the parametrised walks of the host / device comparison
WALKS = (DEFAULT, ((4, 4, 4), (True, False, True)), ((64, 4, 4), (True, False, True)), ((3, 2), (False, True)),
         ((1,), (True,)), ((64,), (True,)), ((5, 5), (True, True)))
CS = (1, 16, 64, 512)


def walk_id(w):
    return 'x'.join(map(str, w[0])) + '-L' + ''.join(str(l + 1) for l, b in enumerate(w[1]) if b)


class WalkRef:
    """the contract over an event list (or, `from_rows`, over per-node entry rows)"""

    def __init__(self, N, src, dst, ts):
        src, dst, ts = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(ts, np.float64)
        E = len(src)
        # entry 2e belongs to src[e], entry 2e + 1 to dst[e]; a node's entries are ordered by time, equal times by entry
        owner = np.stack([src, dst], 1).reshape(-1)
        nbr = np.stack([dst, src], 1).reshape(-1)
        t = np.repeat(ts, 2)
        order = np.lexsort((np.arange(2 * E), t, owner))
        owner, nbr, t = owner[order], nbr[order], t[order]
        cut = np.searchsorted(owner, np.arange(N + 1), side='left')
        self.N = N
        self.t = [t[cut[v]:cut[v + 1]] for v in range(N)]
        self.n = [nbr[cut[v]:cut[v + 1]] for v in range(N)]
        self._memo = {}

    @classmethod
    def from_rows(cls, t_rows, n_rows):
        self = cls.__new__(cls)
        self.N, self.t, self.n, self._memo = len(t_rows), list(t_rows), list(n_rows), {}
        return self

    def trimmed(self, keep_last):
        """every node keeps its last `keep_last` entries"""
        k = int(keep_last)
        return WalkRef.from_rows([r[len(r) - min(k, len(r)):] for r in self.t], [r[len(r) - min(k, len(r)):] for r in self.n])

    def prefix(self, v, t):
        """the neighbour ids of the entries of v with time < t"""
        if not 0 <= v < self.N:
            return self.n[0][:0]
        return self.n[v][:int(np.searchsorted(self.t[v], t, side='left'))]

    def last(self, v, t, F):
        p = self.prefix(v, t)
        return p[max(0, len(p) - F):]

    def ordered(self, src, t, fanout, take, exclude_seen=False, keep_self=False):
        """every candidate of one query in order -> [(id, w), ...]"""
        key = (int(src), float(t), tuple(fanout), tuple(bool(b) for b in take), bool(exclude_seen), bool(keep_self))
        if key in self._memo:
            return self._memo[key]
        w = {}
        level = [int(src)]
        for F, taken in zip(fanout, take):
            nxt = []
            for v in level:
                nxt.extend(self.last(v, t, F).tolist())
            level = nxt
            if taken:
                for v in level:
                    w[v] = w.get(v, 0) + 1
        w.pop(0, None)
        if not keep_self:
            w.pop(int(src), None)
        if exclude_seen:
            for v in set(self.prefix(int(src), t).tolist()):
                w.pop(v, None)
        out = sorted(w.items(), key=lambda kv: (-kv[1], kv[0]))
        self._memo[key] = out
        return out

    def rows(self, src, ts, C, fanout, take, exclude_seen=False, keep_self=False):
        """-> dict(ids int64 [B, C], counts int32 [B, C], n_valid int32 [B], n_distinct int32 [B])"""
        B = len(src)
        ids, counts = np.zeros((B, C), np.int64), np.zeros((B, C), np.int32)
        n_valid, n_distinct = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for i in range(B):
            o = self.ordered(src[i], ts[i], fanout, take, exclude_seen, keep_self)
            k = min(C, len(o))
            ids[i, :k] = [v for v, _ in o[:k]]
            counts[i, :k] = [c for _, c in o[:k]]
            n_valid[i], n_distinct[i] = k, len(o)
        return dict(ids=ids, counts=counts, n_valid=n_valid, n_distinct=n_distinct)


NAMES = ('ids', 'counts', 'n_valid', 'n_distinct')


def assert_same(got, want, what=''):
    """got: a dict of tensors or arrays; want: the reference's dict - array for array"""
    for name in NAMES:
        g = got[name]
        g = g.cpu().numpy() if hasattr(g, 'cpu') else np.asarray(g)
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        np.testing.assert_array_equal(g, want[name], err_msg=f'{what}: {name}')


def library_graph(N, ev, device='cpu', strategy='recent_edges'):
    from www2023tiger_amd.data.graph import Graph
    src, dst, ts = ev[:3]
    eids = ev[3] if len(ev) > 3 else np.arange(1, len(src) + 1, dtype=np.int64)
    return Graph.from_arrays(src, dst, ts, eids, strategy=strategy, max_node_id=N - 1, device=device)


def library_rows(graph, src, ts, C, fanout, take, device='cpu', **flags):
    """hip_ops.walk_candidates with the queries on `device`: the host twin on 'cpu', the kernel elsewhere"""
    import torch
    from www2023tiger_amd import hip_ops
    return hip_ops.walk_candidates(graph, torch.from_numpy(np.ascontiguousarray(src, np.int64)).to(device),
                                   torch.from_numpy(np.ascontiguousarray(ts, np.float64)).to(device), C, fanout=fanout, take=take,
                                   **flags)


# ---- the cases -----------------------------------------------------------------------------------------------------------
_SMALL = {}


def small_case():
    """_cap_ref.small_graph() and 300 queries of _cap_ref.queries -> (N, events, reference, src, ts)"""
    if not _SMALL:
        N, src, dst, ts, eids = _cap_ref.small_graph()
        q, t = _cap_ref.queries(N, 300, float(ts.max()), seed=1)
        _SMALL['case'] = (N, (src, dst, ts, eids), WalkRef(N, src, dst, ts), q, t)
    return _SMALL['case']


def self_loop_queries():
    """sources of the small graph with a self loop, each a little after its first loop -> (src, ts)"""
    _, (src, dst, ts, _), _, _, _ = small_case()
    loops = np.flatnonzero(src == dst)
    first = {}
    for e in loops:
        first.setdefault(int(src[e]), float(ts[e]))
    nodes = np.array(sorted(first), np.int64)[:40]
    return nodes, np.array([first[int(v)] + 1.0 for v in nodes])


SWEEP_PREFIXES = (0, 255, 256, 257, 5000)
SWEEP_FANOUT, SWEEP_TAKE = (4, 4, 4), (True, False, True)
SWEEP_S, SWEEP_U, SWEEP_X, SWEEP_Y, SWEEP_POOL = 1, 2, 3, 4, 50   # source, co-user, the old item, a new item; filler items


def sweep_case(n):
    """A source S whose prefix has exactly n entries: its oldest is an edge with X, the others go to a pool of filler items.
    Its last four items all know the co-user U, and U knows X and Y: X and Y are reached at level 3 ONLY (S -> item -> U ->
    X), X lies in S's prefix far outside its last four entries, Y does not.  -> (N, events, src [1], ts [1])"""
    S, U, X, Y = SWEEP_S, SWEEP_U, SWEEP_X, SWEEP_Y
    pool = np.arange(10, 10 + SWEEP_POOL, dtype=np.int64)
    src, dst = [], []
    if n:
        src.append(S), dst.append(X)
        fill = pool[np.arange(n - 1) % SWEEP_POOL]
        src.extend([S] * (n - 1)), dst.extend(fill.tolist())
        for it in (fill[-4:] if n > 4 else pool[:4]).tolist():
            src.append(it), dst.append(U)
    src.extend([U, U]), dst.extend([X, Y])
    E = len(src)
    ev = (np.array(src, np.int64), np.array(dst, np.int64), np.arange(1, E + 1, dtype=np.float64), np.arange(1, E + 1, dtype=np.int64))
    return 10 + SWEEP_POOL, ev, np.array([S], np.int64), np.array([E + 10.0])


DEGREES = (63, 64, 65)


def degree_case():
    """sources 1, 2, 3 with 63, 64 and 65 entries, all to distinct items -> (N, events, src, ts)"""
    src, dst = [], []
    for s, deg in zip((1, 2, 3), DEGREES):
        src.extend([s] * deg), dst.extend(range(100 * s, 100 * s + deg))
    E = len(src)
    ev = (np.array(src, np.int64), np.array(dst, np.int64), np.arange(1, E + 1, dtype=np.float64), np.arange(1, E + 1, dtype=np.int64))
    return 400, ev, np.array([1, 2, 3], np.int64), np.full(3, E + 1.0)


# (fanout, take): exactly at a cap, and one step past it
AT_CAPS = (((64, 16), (True, True)),             # the frontier cap: 64 * 16 = 1 024
           ((32, 8, 8), (False, False, True)),   # 2 048 endpoints
           ((64,), (True,)), ((64, 16, 2), (False, False, True)))
PAST_CAPS = (((64, 17), (True, True), 'TG_WALK_MAX_FRONTIER'), ((64, 17, 1), (False, False, True), 'TG_WALK_MAX_FRONTIER'),
             ((33, 8, 8), (False, False, True), 'TG_WALK_MAX_ENDPOINTS'),      # 2 112 endpoints
             ((64, 16, 2), (True, False, True), 'TG_WALK_MAX_ENDPOINTS'),      # 64 + 2 048
             ((65,), (True,), 'TG_WALK_MAX_FANOUT'), ((0,), (True,), 'TG_WALK_MAX_FANOUT'),
             ((10, 65), (False, True), 'TG_WALK_MAX_FANOUT'))

STRIDE_N = 70001
STRIDE_FANOUT, STRIDE_TAKE = (32, 8, 8), (False, False, True)   # 2 048 endpoints: the table is at its densest


def stride_case():
    """About 70 000 nodes; one source with 32 items, 8 co-users per item and 8 ends per co-user: 2 048 DISTINCT end ids taken
    from arithmetic progressions with strides 2^8 ... 2^16 (a few offsets each).  Under any power-of-two-masked hash they
    pile into a few residues, so the probe chains are long, with the table as full as it gets.
    -> (N, events, src [1], ts [1])"""
    ends, seen = [], set()
    for off in (0, 1, 3, 7, 12, 100, 200, 255):
        for k in range(16, 7, -1):
            for v in range(off + (1 << k), 70000, 1 << k):
                if v not in seen and v > 400:
                    seen.add(v)
                    ends.append(v)
    ends = np.array(ends[:2048], np.int64)
    assert len(ends) == 2048
    S = 70000
    items, co = np.arange(1, 33, dtype=np.int64), np.arange(100, 356, dtype=np.int64)
    # the source's edges first, the ends' last: the last 8 entries of an item are its co-users, of a co-user its ends
    src = np.concatenate([np.full(32, S), np.repeat(items, 8), np.repeat(co, 8)])
    dst = np.concatenate([items, co, ends])
    E = len(src)
    ev = (src, dst, np.arange(1, E + 1, dtype=np.float64), np.arange(1, E + 1, dtype=np.int64))
    return STRIDE_N, ev, np.array([S], np.int64), np.array([E + 1.0])
