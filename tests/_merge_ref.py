"""Streams, cases and the numpy reference of the late-event tests (tests/test_tcsr_merge_host.py, tests/test_hip_tcsr_merge.py,
tests/test_hip_observe_late.py).

The reference makes no library call.  Per row: the old row followed by the owner's new entries in ascending j (j = 2e: event e
seen from src, j = 2e + 1: seen from dst), then np.argsort(kind='stable') on the times - numpy compares with '<', so -0.0 and
+0.0 tie and keep that order.  Every comparison against it is exact, on the raw bits."""
import ctypes as C

import numpy as np

from _append_ref import NAMES, assert_same, host_build, stream  # noqa: F401  (re-exported)

DT = (np.int64, np.int64, np.float64, np.int64)


def as_batch(ev):
    return tuple(np.ascontiguousarray(a, dtype=dt) for a, dt in zip(ev, DT))


def np_merge(h, N, new):
    """host arrays h = (indptr [N0 + 1], ts, nbr, eid) merged with the batch `new` over N >= N0 nodes -> the four arrays"""
    indptr0, ts0, nbr0, eid0 = h
    N0 = len(indptr0) - 1
    src, dst, ts, eid = new
    n = len(src)
    j = np.arange(2 * n)
    e, f = j >> 1, (j & 1).astype(bool)
    owner = np.where(f, dst[e], src[e]) if n else np.empty(0, dtype=np.int64)
    n_ts, n_nbr = ts[e], np.where(f, src[e], dst[e]).astype(np.int32)
    n_eid = (eid[e].astype(np.uint32) | (f.astype(np.uint32) << np.uint32(31))).view(np.int32)
    by_owner = np.argsort(owner, kind='stable')          # ascending j inside an owner
    first = np.searchsorted(owner[by_owner], np.arange(N + 1))
    P = len(ts0) + 2 * n
    out = (np.empty(N + 1, dtype=np.int64), np.empty(P, dtype=np.float64), np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32))
    q = 0
    for v in range(N):
        lo, hi = (indptr0[v], indptr0[v + 1]) if v < N0 else (len(ts0), len(ts0))
        mine = by_owner[first[v]:first[v + 1]]
        t = np.concatenate([ts0[lo:hi], n_ts[mine]])
        perm = np.argsort(t, kind='stable')
        out[0][v] = q
        out[1][q:q + len(t)] = t[perm]
        out[2][q:q + len(t)] = np.concatenate([nbr0[lo:hi], n_nbr[mine]])[perm]
        out[3][q:q + len(t)] = np.concatenate([eid0[lo:hi], n_eid[mine]])[perm]
        q += len(t)
    out[0][N] = q
    assert q == P
    return out


def random_tcsr(N, P, seed, *, t_hi=None, rows=None):
    """host T-CSR arrays of exactly P entries that belong to no event list (any P, odd ones included): a random partition
    into N rows (rows: restrict the owners to these ids), floored ascending times per row, random neighbours and eids"""
    rs = np.random.RandomState(seed)
    owner = np.sort(rs.choice(rows, P) if rows is not None else rs.randint(0, N, P))
    indptr = np.searchsorted(owner, np.arange(N + 1)).astype(np.int64)
    ts = np.floor(rs.uniform(0, t_hi if t_hi is not None else max(P / 6.0, 4.0), P))
    ts = ts[np.lexsort((ts, owner))]
    return (indptr, np.ascontiguousarray(ts), rs.randint(0, N, P).astype(np.int32),
            rs.randint(-2 ** 31, 2 ** 31, P).astype(np.int32))


def late_batch(N, n, seed, t_lo, t_hi, *, hub=None, ids_from=0, floor=True):
    """n events in no order: ids in [ids_from, N), times uniform in [t_lo, t_hi) (floored: duplicates), some self loops;
    hub: that node owns most entries"""
    rs = np.random.RandomState(seed)
    src, dst = rs.randint(ids_from, N, n).astype(np.int64), rs.randint(ids_from, N, n).astype(np.int64)
    loops = rs.uniform(size=n) < 0.05
    dst[loops] = src[loops]
    if hub is not None:
        src[rs.uniform(size=n) < 0.95] = hub
        dst[rs.uniform(size=n) < 0.85] = hub
    ts = rs.uniform(t_lo, t_hi, n)
    return as_batch((src, dst, np.floor(ts) if floor else ts, rs.randint(0, 2 ** 31, n)))


def _events(N, E, seed, ts):
    rs = np.random.RandomState(seed)
    return as_batch((rs.randint(0, N, E), rs.randint(0, N, E), ts, rs.randint(0, 2 ** 31, E)))


def _cases():
    """name -> (N0, N, old events (time ordered), batch)"""
    c = {}
    s = stream(50, 400, seed=1)
    old = as_batch(tuple(a[:300] for a in s))
    t_hi = float(s[2][299])
    c['empty-old'] = (50, 50, as_batch(tuple(a[:0] for a in s)), late_batch(50, 120, 2, 0, 40))
    c['n0'] = (50, 50, old, as_batch(tuple(a[:0] for a in s)))
    c['all-before'] = (50, 50, old, late_batch(50, 90, 3, -500, -1))
    c['all-after-ordered'] = (50, 50, old, as_batch(tuple(a[300:] for a in s)))   # what tg_tcsr_append takes
    c['reversed'] = (50, 50, old, as_batch(tuple(a[300:][::-1] for a in s)))
    c['inside'] = (50, 50, old, late_batch(50, 150, 4, 0, t_hi + 3))
    c['all-equal'] = (9, 9, _events(9, 60, 5, np.full(60, 5.0)), _events(9, 45, 6, np.full(45, 5.0)))
    z = np.array([-0.0, 0.0, -1.0, 1.0, 0.0, -0.0])
    rs = np.random.RandomState(7)
    c['signed-zeros'] = (6, 6, _events(6, 80, 8, np.sort(z[rs.randint(0, 6, 80)])), _events(6, 70, 9, z[rs.randint(0, 6, 70)]))
    w = np.array([-np.inf, np.inf, 0.0, 3.0, -3.0, 1e300, -1e300])
    c['inf'] = (12, 12, _events(12, 90, 10, np.sort(w[rs.randint(0, 7, 90)])), _events(12, 64, 11, w[rs.randint(0, 7, 64)]))
    loop = as_batch((np.full(40, 2), np.full(40, 2), np.floor(np.arange(40) / 4.0), np.arange(40)))
    c['self-loops'] = (4, 4, loop, as_batch((np.full(30, 2), np.full(30, 2), np.floor(rs.uniform(-1, 11, 30)), np.arange(40, 70))))
    pair = lambda k, t, e0: as_batch((np.full(k, 1), np.full(k, 3), t, np.arange(e0, e0 + k)))
    c['multi-edges'] = (5, 5, pair(50, np.floor(np.arange(50) / 5.0), 0), pair(40, np.floor(rs.uniform(0, 10, 40)), 50))
    sh = stream(300, 2000, seed=12, hub=7)
    c['hub'] = (300, 300, as_batch(sh), late_batch(300, 900, 13, 0, float(sh[2][-1]) + 1, hub=7))
    c['growth'] = (50, 77, old, late_batch(77, 130, 14, 0, t_hi))
    c['growth-new-ids-only'] = (50, 64, old, late_batch(64, 40, 15, -5, t_hi / 2, ids_from=50))
    c['growth-n0'] = (50, 51, old, as_batch(tuple(a[:0] for a in s)))
    return c


CASES = _cases()


def concat(old, new):
    return tuple(np.concatenate([a, b]) for a, b in zip(old, new))


def host_merge(h, N, new):
    """tg_tcsr_merge_host on host arrays h over N >= N0 nodes -> (rc, arrays)"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    n, N0 = len(new[0]), len(h[0]) - 1
    P = len(h[1]) + 2 * n
    out = (np.empty(N + 1, dtype=np.int64), np.empty(P, dtype=np.float64), np.empty(P, dtype=np.int32),
           np.empty(P, dtype=np.int32))
    g = TgTcsr(N0, len(h[1]), *(ptr(a) for a in h))
    rc = lib.tg_tcsr_merge_host(C.byref(g), N, n, *(ptr(a) for a in new), *(ptr(a) for a in out))
    return rc, out
