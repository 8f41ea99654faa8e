"""Streams and the reference of the T-CSR extension tests (tests/test_tcsr_append_host.py, tests/test_hip_tcsr_append.py).

The reference is tg_tcsr_build_host over the old events followed by the new ones; every comparison is exact."""
import ctypes as C

import numpy as np

NAMES = ('indptr', 'ts', 'nbr', 'eid')


def stream(N, E, seed=0, *, hub=None, T=None):
    """E time-ordered events over ids [0, N): floored timestamps (duplicates), some self loops, arbitrary 31-bit edge ids
    (the largest one included).  hub: that node is the source of 95 % and the destination of 85 % of the events - it owns
    90 % of the entries, many of them self loops."""
    rs = np.random.RandomState(seed)
    src, dst = rs.randint(0, N, E).astype(np.int64), rs.randint(0, N, E).astype(np.int64)
    loops = rs.uniform(size=E) < 0.05
    dst[loops] = src[loops]
    if hub is not None:
        src[rs.uniform(size=E) < 0.95] = hub
        dst[rs.uniform(size=E) < 0.85] = hub
    ts = np.floor(np.sort(rs.uniform(0, T if T is not None else max(E / 3.0, 4.0), E)))
    eids = rs.randint(0, 2 ** 31, E).astype(np.int64)
    if E:
        eids[rs.randint(0, E)] = 0x7FFFFFFF
    return src, dst, ts, eids


TINY = (np.array([3, 3, 1]), np.array([3, 2, 3]), np.array([1.0, 1.0, 2.0]), np.array([1, 2, 3]))


def equal_t_last(N=40, E0=300, n=100):
    """the first 30 new events carry the timestamp of the last old one"""
    s = list(stream(N, E0 + n, seed=11))
    s[2] = s[2].copy()
    s[2][E0 - 20:E0 + 30] = s[2][E0 - 1]
    s[2][E0 + 30:] = np.maximum(s[2][E0 + 30:], s[2][E0 - 1])
    assert np.all(s[2][1:] >= s[2][:-1])
    return tuple(s)


# name -> (N, E0, full stream); the new events are the stream past E0
CASES = {
    'N2-E0-n1': (2, 0, stream(2, 1, seed=1)),
    'tiny-1+2': (5, 1, TINY),   # the `tiny` stream of test_device_tcsr_build_equals_host_build: a self loop, duplicate times
    'N65-E1-n200': (65, 1, stream(65, 201, seed=2)),
    'N1000-E1023-n1025': (1000, 1023, stream(1000, 2048, seed=3)),
    'N9228-E5000-n1024': (9228, 5000, stream(9228, 6024, seed=4)),
    'hub-one-workgroup': (300, 2000, stream(300, 4000, seed=5, hub=7)),    # 2 n = 4000: about 3600 cut points coincide
    'hub-radix': (300, 3000, stream(300, 5600, seed=6, hub=7)),            # 2 n = 5200: about 4700 cut points coincide
    'first-ts-equal-t-last': (40, 300, equal_t_last()),
    'n0': (30, 200, stream(30, 200, seed=7)),
}


def cut(case):
    """-> N, (old events), (new events)"""
    N, E0, s = CASES[case] if isinstance(case, str) else case
    s = tuple(np.ascontiguousarray(a, dtype=dt) for a, dt in zip(s, (np.int64, np.int64, np.float64, np.int64)))
    return N, tuple(a[:E0] for a in s), tuple(a[E0:] for a in s)


def host_build(N, src, dst, ts, eids):
    """tg_tcsr_build_host -> (indptr, ts, nbr, eid)"""
    from www2023tiger_amd._lib import check, lib, ptr
    E = len(src)
    h = (np.empty(N + 1, dtype=np.int64), np.empty(2 * E, dtype=np.float64), np.empty(2 * E, dtype=np.int32),
         np.empty(2 * E, dtype=np.int32))
    check(lib.tg_tcsr_build_host(E, ptr(src), ptr(dst), ptr(ts), ptr(eids), N, *(ptr(a) for a in h)), 'tg_tcsr_build_host')
    return h


def reference(N, old, new):
    return host_build(N, *(np.concatenate([a, b]) for a, b in zip(old, new)))


def host_append(N, h, new):
    """tg_tcsr_append_host on host arrays h -> (rc, arrays)"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    n = len(new[0])
    P = len(h[1]) + 2 * n
    out = (np.empty(N + 1, dtype=np.int64), np.empty(P, dtype=np.float64), np.empty(P, dtype=np.int32),
           np.empty(P, dtype=np.int32))
    g = TgTcsr(N, len(h[1]), *(ptr(a) for a in h))
    rc = lib.tg_tcsr_append_host(C.byref(g), n, *(ptr(a) for a in new), *(ptr(a) for a in out))
    return rc, out


def assert_same(got, want, what=''):
    for a, b, nm in zip(got, want, NAMES):
        assert a.dtype == b.dtype and a.shape == b.shape, f'{what} {nm}: {a.dtype}{a.shape} against {b.dtype}{b.shape}'
        np.testing.assert_array_equal(a.view(np.int64 if a.itemsize == 8 else np.int32),
                                      b.view(np.int64 if b.itemsize == 8 else np.int32), err_msg=f'{what} {nm}')
