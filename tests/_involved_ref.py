"""Numpy reference and shared inputs of the involved-list tests (tests/test_involved_host.py, tests/test_hip_involved.py,
tests/test_hip_rank_restarts.py): the set GraphCollator.collate_memory_nodes flags, restated over the oracle's sampler -
the queries, their K slots (padding id 0 included) and, with two layers, the K slots of every hop-1 slot at the slot's
FLOAT32 time - then np.unique, a set difference against a bool `uptodate`, and np.float32(ts.min())."""
import numpy as np

F32_T = float(2 ** 27 + 3)     # an event time float32 cannot hold: it rounds DOWN to 2^27 (spacing 16)
F32_BETWEEN = float(2 ** 27 + 1)  # another event of the same neighbour between the rounded and the unrounded value
F32_QUERY_T = float(2 ** 27 + 100)
ISOLATED = 5                   # a node of the hand-made graphs without any event


def oracle_graph(ev, strategy):
    from oracle import tiger_oracle as O
    return O.OracleGraph(ev['src'], ev['dst'], ev['ts'], ev['eids'], strategy=strategy, max_node_id=ev['n_nodes'] - 1)


def numpy_involved(og, nids, ts, K, n_layers, strategy, round_hop2=True):
    """sorted unique involved ids of the (nids[q], ts[q]) queries.  round_hop2=False searches the second hop at the
    unrounded float64 entry times instead (what the collator does NOT do; recent_edges only) - to show that a case tells
    the two apart."""
    nids, ts = np.asarray(nids, np.int64), np.asarray(ts, np.float64)
    if len(nids) == 0:
        return np.zeros(0, np.int64)
    l_n, _, l_t, _ = og.sample_temporal_neighbor(nids, ts, K, strategy=strategy)
    parts = [nids, l_n.ravel()]
    if n_layers == 2:
        t2 = l_t.ravel().astype(np.float64)
        if not round_hop2:
            assert strategy == 'recent_edges'
            t2 = np.zeros((len(nids), K))
            for q, (v, t) in enumerate(zip(nids, ts)):
                lo, hi = og.find_before(int(v), t)
                sel = np.arange(max(lo, hi - K), hi)
                t2[q, K - len(sel):] = og.ts[sel]
            t2 = t2.ravel()
        parts.append(og.sample_temporal_neighbor(l_n.ravel(), t2, K, strategy=strategy)[0].ravel())
    return np.unique(np.concatenate(parts))


_REF = {}


def reference(name, ev, nids, ts, K, n_layers, strategy):
    """numpy_involved, computed once per (graph, queries, K, layers, strategy) and shared between the test modules"""
    key = (name, len(nids), K, n_layers, strategy)
    if key not in _REF:
        _REF[key] = numpy_involved(oracle_graph(ev, strategy), nids, ts, K, n_layers, strategy)
    return _REF[key]


def expected(involved, ts, upto_bool):
    """-> (ids listed, count, tmin float32, uptodate afterwards) for a bool uptodate array"""
    ids = np.setdiff1d(involved, np.nonzero(upto_bool)[0])
    after = upto_bool.copy()
    after[involved] = True
    return ids, len(ids), np.float32(np.min(ts)) if len(ts) else None, after


# ---- bitmaps ---------------------------------------------------------------------------------------------------------------
def to_bitmap(upto_bool):
    """bool [n_nodes] -> int64 words, bit i of word w = node 64 w + i"""
    W = (len(upto_bool) + 63) // 64
    b = np.zeros(W * 64, dtype=np.uint8)
    b[:len(upto_bool)] = upto_bool
    return np.packbits(b, bitorder='little').view(np.int64).copy()


def from_bitmap(words, n_nodes):
    return np.unpackbits(np.asarray(words).view(np.uint8), bitorder='little')[:n_nodes].astype(bool)


def uptodate_states(n_nodes, seed=0):
    """empty, full, a random half"""
    return dict(empty=np.zeros(n_nodes, bool), full=np.ones(n_nodes, bool),
                half=np.random.RandomState(seed + n_nodes).rand(n_nodes) < 0.5)


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def stream_events():
    """the 76-node graph of bench.make_stream(60, 15, 200): integer times, so equal times occur"""
    import bench
    st = bench.make_stream(60, 15, 200, 5000.0, seed=0, with_efeats=False)
    return dict(src=st['src'], dst=st['dst'], ts=st['ts'], eids=st['eids'], n_nodes=st['n_nodes'])


def hand_events(n_nodes, E=300, seed=0):
    """Hand-made events over ids 1 .. n_nodes - 1 (n_nodes 64, 65, 129: the edges of a bitmap word).  Random events between
    nodes 6 .. n_nodes - 1 at small integer times (many equal), a few of nodes 1 and 2 among them, node ISOLATED in none;
    then the float32 case: (3, 2) at F32_BETWEEN and (1, 2) at F32_T - node 3 has no other event, F32_T rounds down to 2^27
    in float32, so the second hop of the slot (2, float32(F32_T)) of a query of node 1 must NOT see node 3, and a search at
    the unrounded time would.  The last event touches node n_nodes - 1."""
    rs = np.random.RandomState(seed + n_nodes)
    a = rs.randint(6, n_nodes, E)
    b = rs.randint(6, n_nodes, E)
    a[:12] = np.repeat([1, 2], 6)
    ts = np.sort(rs.randint(1, 60, E)).astype(np.float64)
    src = np.concatenate([a, [3, 1, n_nodes - 1]]).astype(np.int64)
    dst = np.concatenate([b, [2, 2, 6]]).astype(np.int64)
    ts = np.concatenate([ts, [F32_BETWEEN, F32_T, F32_T + 50.0]])
    assert np.float32(F32_T) <= F32_BETWEEN < F32_T and not (src == ISOLATED).any() and not (dst == ISOLATED).any()
    return dict(src=src, dst=dst, ts=ts, eids=np.arange(1, len(src) + 1, dtype=np.int64), n_nodes=n_nodes)


GRAPHS = {'stream76': stream_events, 'hand64': lambda: hand_events(64), 'hand65': lambda: hand_events(65),
          'hand129': lambda: hand_events(129)}
_EV = {}


def events(name):
    if name not in _EV:
        _EV[name] = GRAPHS[name]()
    return _EV[name]


def queries(ev, Q, seed=0):
    """Q (node, time) queries.  In front, as far as Q reaches: (hand-made graphs) the float32 case; the pad id 0; node
    n_nodes - 1 after everything; a node with no event before its time; a time equal to an event's time (strict cut: that
    event does not count); a query twice.  Then random nodes at event times, between them and after everything."""
    rs = np.random.RandomState(seed + 17 * Q + ev['n_nodes'])
    n_nodes, t_last = ev['n_nodes'], float(ev['ts'].max())
    k = len(ev['ts']) // 2
    first = [(1, F32_QUERY_T)] if t_last > 2 ** 27 else []
    first += [(0, t_last + 1.0), (n_nodes - 1, t_last + 1.0), (int(ev['src'][k]), float(ev['ts'][0])),
              (int(ev['src'][k]), float(ev['ts'][k])), (int(ev['dst'][k]), float(ev['ts'][k]) + 0.5)]
    first += [first[-1]]
    if t_last > 2 ** 27:
        first += [(ISOLATED, t_last), (2, F32_T)]
    nid = rs.randint(0, n_nodes, Q).astype(np.int64)
    pool = np.concatenate([ev['ts'], ev['ts'] + 0.5, [t_last + 10.0, 0.0]])
    ts = pool[rs.randint(0, len(pool), Q)].astype(np.float64)
    for i, (v, t) in enumerate(first[:Q]):
        nid[i], ts[i] = v, t
    return nid, ts
