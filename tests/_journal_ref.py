"""A numpy reference for the journal kernels (tg_journal.hip): packing rows of a T-CSR, splicing them back, scattering
per-node rows and bits - each written row by row with Python loops and concatenation, nothing shared with the library -
and the cases that tests/test_journal_host.py (host twins) and tests/test_hip_journal_ops.py (device kernels) both run."""
import numpy as np
import torch

ROW_COUNTS = (0, 1, 2, 63, 64, 65, 2047, 2048, 2049)
N_BIG, HUB, HUB_LEN = 2100, 1000, 5000
DTYPES = (np.int64, np.float64, np.int32, np.int32)


def rows_of(arrays):
    """the T-CSR as a list of per-row (ts, nbr, eid) triples"""
    ip = arrays[0]
    return [tuple(a[ip[v]:ip[v + 1]] for a in arrays[1:]) for v in range(len(ip) - 1)]


def arrays_of(rows):
    """the four arrays of a list of per-row triples"""
    lens = [len(r[0]) for r in rows]
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cat = lambda k, dt: np.concatenate([r[k] for r in rows]).astype(dt) if rows and ip[-1] else np.zeros(0, dtype=dt)
    return ip, cat(0, np.float64), cat(1, np.int32), cat(2, np.int32)


def random_row(rs, n, N, t0=0.0):
    return (np.sort(rs.rand(n) * 100.0 + t0), rs.randint(0, N, n).astype(np.int32),
            (rs.randint(1, 1 << 20, n) | (rs.randint(0, 2, n) << 31)).astype(np.uint32).view(np.int32))


def random_graph(N, seed, hub=None, empty=0.3):
    """N rows of 0 to 6 entries (a share `empty` of them empty), row `hub` with HUB_LEN entries"""
    rs = np.random.RandomState(seed)
    deg = np.where(rs.rand(N) < empty, 0, rs.randint(1, 7, N))
    if hub is not None:
        deg[hub] = HUB_LEN
    return arrays_of([random_row(rs, int(n), N) for n in deg])


def pick_rows(N, D, seed, must=()):
    """D distinct ascending row ids of [0, N), those of `must` among them as far as D allows"""
    rs = np.random.RandomState(seed)
    must = list(must)[:D]
    rest = np.setdiff1d(np.arange(N), must)
    return np.sort(np.concatenate([must, rs.choice(rest, D - len(must), replace=False)])).astype(np.int32)


def pack_ref(arrays, rows):
    """-> off int64 [D + 1], ts, nbr, eid of the listed rows, one after the other"""
    per = rows_of(arrays)
    got = [per[v] for v in rows]
    ip, ts, nbr, eid = arrays_of(got)
    return ip, ts, nbr, eid


def splice_ref(arrays, n_new, rows, off, pack):
    """-> the four arrays over n_new ids: row rows[j] is pack row j, every other row the old one (empty beyond the old count)"""
    per = rows_of(arrays)
    empty = tuple(np.zeros(0, dtype=dt) for dt in DTYPES[1:])
    per = per + [empty] * (n_new - len(per))
    for j, v in enumerate(rows):
        per[v] = tuple(a[off[j]:off[j + 1]] for a in pack)
    return arrays_of(per)


def rewritten(arrays, rows, seed, n_new=None):
    """another graph: the listed rows get new contents (some empty, some longer, the hub - if listed - another 4500), the rest
    stay; ids at and beyond the old count are empty unless listed"""
    rs = np.random.RandomState(seed)
    N = len(arrays[0]) - 1
    n_new = N if n_new is None else n_new
    per = rows_of(arrays) + [tuple(np.zeros(0, dtype=dt) for dt in DTYPES[1:])] * (n_new - N)
    for v in rows:
        n = 4500 if v == HUB and N == N_BIG else int(rs.randint(0, 9))
        per[v] = random_row(rs, n, n_new, t0=100.0)
    return arrays_of(per)


def scatter_ref(dst, ids, src):
    out = dst.copy()
    for j, i in enumerate(ids):
        if 0 <= i < len(out):
            out[i] = src[j]
    return out


def bit_scatter_ref(bits, ids, flags, n_ids):
    """bits: int64 words; -> the words with bit ids[j] = flags[j] != 0"""
    b = np.unpackbits(bits.view(np.uint8), bitorder='little').copy()
    for j, i in enumerate(ids):
        if 0 <= i < n_ids:
            b[i] = 1 if flags[j] else 0
    return np.packbits(b, bitorder='little').view(np.int64)


def tensors(arrays, device='cpu'):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays)


def assert_arrays(got, ref, what=''):
    """four tensors against four numpy arrays: dtype, shape and bits"""
    for a, b, name in zip(got, ref, ('indptr', 'ts', 'nbr', 'eid')):
        a = a.cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape, f'{what}: {name} {a.dtype}{a.shape} != {b.dtype}{b.shape}'
        v = np.int64 if a.dtype == np.float64 else a.dtype
        assert np.array_equal(a.view(v), b.view(v)), f'{what}: {name}'


_CACHE = {}


def big():
    """about 2 100 nodes: empty rows, one hub row of 5 000 entries (more than two tiles of 2 048)"""
    if 'big' not in _CACHE:
        _CACHE['big'] = random_graph(N_BIG, 7, hub=HUB)
    return _CACHE['big']


def empty_graph(N):
    return (np.zeros(N + 1, dtype=np.int64),) + tuple(np.zeros(0, dtype=dt) for dt in DTYPES[1:])


def graph_cases():
    """name -> (old arrays, n_new, rows, new arrays): `new` is `old` with the listed rows rewritten.  The first and the last
    row and the hub are listed wherever D allows."""
    if 'cases' in _CACHE:
        return _CACHE['cases']
    out = {}
    old = big()
    ends = (0, N_BIG - 1, HUB)
    for D in ROW_COUNTS:
        rows = pick_rows(N_BIG, D, 100 + D, must=ends)
        out[f'D{D}'] = (old, N_BIG, rows, rewritten(old, rows, 200 + D))
    rows = np.arange(N_BIG, dtype=np.int32)
    out['all-dirty'] = (old, N_BIG, rows, rewritten(old, rows, 1))
    n_new = N_BIG + 130
    rows = np.sort(np.concatenate([pick_rows(N_BIG, 40, 2, must=ends), [N_BIG, N_BIG + 64, n_new - 1]])).astype(np.int32)
    out['grown-dirty-new-ids'] = (old, n_new, rows, rewritten(old, rows, 3, n_new))
    rows = pick_rows(N_BIG, 40, 4, must=ends)
    out['grown-untouched-new-ids'] = (old, n_new, rows, rewritten(old, rows, 5, n_new))
    small = random_graph(65, 9)
    rows = pick_rows(65, 5, 6, must=(0, 64))
    out['small'] = (small, 65, rows, rewritten(small, rows, 7))
    e = empty_graph(70)
    rows = pick_rows(70, 9, 8, must=(0, 69))
    out['empty-old'] = (e, 70, rows, rewritten(e, rows, 9))
    rows = np.array([3, 69, 70, 199], dtype=np.int32)
    out['empty-old-grown'] = (e, 200, rows, rewritten(e, rows, 10, 200))
    out['empty-old-nothing'] = (e, 70, np.zeros(0, dtype=np.int32), e)
    _CACHE['cases'] = out
    return out


CASE_NAMES = tuple(f'D{D}' for D in ROW_COUNTS) + ('all-dirty', 'grown-dirty-new-ids', 'grown-untouched-new-ids', 'small',
                                                   'empty-old', 'empty-old-grown', 'empty-old-nothing')


def events(N, E, seed, t0=0.0):
    """a time-ordered stream of E events among the ids [1, N): src, dst, ts, eids"""
    rs = np.random.RandomState(seed)
    return (rs.randint(1, N, E).astype(np.int64), rs.randint(1, N, E).astype(np.int64),
            t0 + np.sort(rs.rand(E) * 50.0), np.arange(1, E + 1, dtype=np.int64))


def children(g, N, E):
    """name -> a child of the library Graph `g` (built over events(N, E, ...)): what the model's writers swap in"""
    s, d, t, e = events(N, 90, 21, t0=60.0)
    late = events(N, 40, 22, t0=10.0)
    return {
        'extended': g.extended(s, d, t, e + E),
        'merged': g.merged(late[0], late[1], late[2], late[3] + E),
        'trimmed': g.trimmed(before=12.0, keep_last=3),
        'without': g.without(nodes=[5, 9, 33], eids=list(range(10, 30))),
    }


# ---- row widths of the scatter: bytes per row -> (dtype, trailing shape) ---------------------------------------------------
SCATTER_ROWS = {1: (torch.uint8, ()), 4: (torch.float32, ()), 8: (torch.float64, ()), 16: (torch.float32, (4,)),
                32: (torch.float32, (8,)), 64: (torch.float32, (16,)), 688: (torch.float32, (172,)), 48: (torch.int32, (3, 4))}


def scatter_case(nbytes, n_dst, D, seed):
    """-> dst before, ids int32 [D] (ascending, distinct), src [D] rows"""
    dt, shape = SCATTER_ROWS[nbytes]
    g = torch.Generator().manual_seed(seed)
    make = lambda n: (torch.randint(0, 250, (n,) + shape, generator=g).to(dt) if dt in (torch.uint8, torch.int32)
                      else torch.randn((n,) + shape, generator=g).to(dt))
    ids = pick_rows(n_dst, D, seed, must=(0, n_dst - 1))
    return make(n_dst), torch.from_numpy(ids), make(D)
