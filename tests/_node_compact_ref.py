"""The reference of the node-id compaction tests: numpy, a dict and `Graph.from_arrays` on the host.

Sizes.  The issue's list - the word (64 ids), wavefront (128) and 2 048 edges and the select tile of 2 048 words = 131 072
ids - and the edges of THIS implementation that it does not contain: a thread of the plan owns 8 words = 512 ids, a
wavefront 64 threads = 32 768 ids, a workgroup one tile of 131 072 ids; 262 149 ids span three tiles, so that one WHOLE
tile (the second) can be dropped."""
import numpy as np

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 131071, 131072, 131073, 140000)
OWN_SIZES = (511, 512, 513, 32767, 32768, 32769, 262149)
EDGES = (64, 128, 512, 2048, 32768, 131072, 262144)
DROPS = ('none', 'one', 'last', 'all_but_0', 'alternating', 'word', 'tile', 'edges')


def drop_ids(N, name):
    """the ids that leave, int64, ascending; never 0"""
    if name == 'none' or N < 2:
        ids = []
    elif name == 'one':
        ids = [max(1, N // 2)]
    elif name == 'last':
        ids = [N - 1]
    elif name == 'all_but_0':
        ids = np.arange(1, N)
    elif name == 'alternating':
        ids = np.arange(1, N, 2)
    elif name == 'word':   # one whole 64-bit word of the bitmap (the first one keeps id 0)
        ids = np.arange(64, 128) if N >= 128 else np.arange(1, min(N, 64))
    elif name == 'tile':   # one whole tile of 2048 words (the first one keeps id 0)
        ids = np.arange(131072, 262144) if N >= 262144 else np.arange(1, min(N, 131072))
    elif name == 'edges':  # the ids each side of every edge
        ids = sorted({i for e in EDGES for i in (e - 1, e, e + 1) if 1 <= i < N})
    else:
        raise KeyError(name)
    return np.asarray(ids, dtype=np.int64)


def bitmap(ids, n_ids, words=None):
    """int64 words over n_ids ids with the bits of `ids` set"""
    W = (n_ids + 63) // 64 if words is None else words
    bits = np.zeros(W, dtype=np.uint64)
    ids = np.asarray(ids, dtype=np.int64)
    np.bitwise_or.at(bits, ids >> 6, np.uint64(1) << (ids & 63).astype(np.uint64))
    return bits.view(np.int64)


def unpack(bits, n_ids):
    """bool [n_ids] of an int64 bitmap"""
    b = np.asarray(bits).view(np.uint64)
    return ((b[np.arange(n_ids) >> 6] >> (np.arange(n_ids) & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def remap_ref(N, drop):
    """(remap int32 [N], old_of int32 [n_new])"""
    keep = np.ones(N, dtype=bool)
    keep[drop] = False
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return remap, np.nonzero(keep)[0].astype(np.int32)


def events(num_node, drop, E=3000, seed=0):
    """A time-ordered stream over the ids of [1, num_node) that stay: a few HUB ids take half of the endpoints, the others
    are spread thinly, so hub rows stand next to runs of thousands of empty rows at the large sizes.  Equal timestamps
    and self loops occur.  -> (src, dst, ts, eids)"""
    rs = np.random.RandomState(seed)
    alive = np.setdiff1d(np.arange(1, num_node), drop)
    if len(alive) == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy(), np.zeros(0, dtype=np.float64), z.copy()
    E = min(E, 40 * len(alive))
    hubs = alive[np.unique(np.concatenate([[0, len(alive) - 1], rs.randint(0, len(alive), 3)]))]
    pick = lambda: np.where(rs.rand(E) < 0.5, hubs[rs.randint(0, len(hubs), E)], alive[rs.randint(0, len(alive), E)])
    src, dst = pick().astype(np.int64), pick().astype(np.int64)
    ts = np.sort(np.floor(rs.rand(E) * E / 2))   # equal times
    return src, dst, ts.astype(np.float64), np.arange(1, E + 1, dtype=np.int64)


def graph_of(ev, num_node):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(*ev, strategy='recent_edges', seed=0, max_node_id=num_node - 1)


def compacted_ref(ev, remap, n_graph_new):
    """the four host arrays of `from_arrays` over the events with src / dst passed through remap"""
    r = remap.astype(np.int64)
    return graph_of((r[ev[0]], r[ev[1]], ev[2], ev[3]), n_graph_new)._host_tcsr()


def bitmap_compact_ref(bits, n_in, old_of):
    """new bit j = old bit old_of[j] over the kept ids below n_in"""
    old = old_of[old_of < n_in]
    return bitmap(np.nonzero(unpack(bits, n_in)[old])[0], len(old))
