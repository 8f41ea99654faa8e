"""Streams and the reference of the node-growth tests (tests/test_tcsr_grow_host.py, tests/test_hip_tcsr_grow.py).

A case is (N0, N1, old events, new events): the old events name ids below N0, the new ones ids below N1.  The reference is
tg_tcsr_build_host over the old events followed by the new ones with N1 nodes; every comparison is exact."""
import ctypes as C

import numpy as np

from _append_ref import NAMES, assert_same, host_build, stream  # noqa: F401

DT = (np.int64, np.int64, np.float64, np.int64)


def _typed(ev):
    return tuple(np.ascontiguousarray(a, dtype=dt) for a, dt in zip(ev, DT))


def grow_case(N0, N1, E0, n, seed, *, frac_new=0.3):
    """E0 old events over [0, N0) followed by n new ones over [0, N1) of which about frac_new name an id in [N0, N1) on
    either side (both sides now and then: self loops on new nodes and new-new edges included); time-ordered across the cut"""
    s, d, t, e = stream(N1, E0 + n, seed=seed)
    rs = np.random.RandomState(seed + 1000)
    s[:E0] %= N0
    d[:E0] %= N0
    if N1 > N0:
        for a in (s, d):
            old = rs.uniform(size=n) >= frac_new
            a[E0:][old] %= N0
            a[E0:][~old] = N0 + a[E0:][~old] % (N1 - N0)
    ev = _typed((s, d, t, e))
    return N0, N1, tuple(a[:E0] for a in ev), tuple(a[E0:] for a in ev)


def hand_case(N0, N1, E0, new_src, new_dst, seed=3):
    """E0 random old events over [0, N0) and the given new (src, dst) pairs after them"""
    s, d, t, e = _typed(stream(N0, E0, seed=seed))
    n = len(new_src)
    t_last = t[-1] if E0 else 0.0
    new = _typed((new_src, new_dst, t_last + np.arange(n) // 2, 7 + np.arange(n)))
    return N0, N1, (s, d, t, e), new


EMPTY = _typed(([], [], [], []))

# name -> (N0, N1, old, new)
CASES = {
    'N1-to-2': grow_case(1, 2, 5, 9, seed=21),
    'N2-to-3': grow_case(2, 3, 7, 12, seed=22),
    'N255-to-257': grow_case(255, 257, 400, 300, seed=23, frac_new=0.1),
    'no-events': (40, 47, _typed(stream(40, 120, seed=24)), EMPTY),
    'no-events-empty-graph': (3, 9, EMPTY, EMPTY),
    'new-only-dst': hand_case(20, 22, 60, [1, 2, 3], [20, 21, 20]),
    'new-only-src': hand_case(20, 22, 60, [21, 20, 21], [4, 5, 6]),
    'self-loop-on-new': hand_case(20, 21, 60, [20, 20, 3], [20, 20, 20]),
    'gap': hand_case(20, 26, 60, [25, 2, 25], [1, 25, 25]),       # only id N0 + 5 appears: five empty rows between
    'twice-in-batch': hand_case(30, 34, 80, [31, 4, 31, 33], [2, 31, 33, 33]),
    'no-growth': grow_case(50, 50, 200, 90, seed=25),
    'old-graph-empty': grow_case(4, 9, 0, 30, seed=26),
}


def reference(N1, old, new):
    return host_build(N1, *(np.concatenate([a, b]) for a, b in zip(old, new)))


def host_append_grow(N0, N1, h, new, entry='tg_tcsr_append_grow_host'):
    """tg_tcsr_append_grow_host on host arrays h -> (rc, arrays)"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    n = len(new[0])
    P = len(h[1]) + 2 * n
    rows = N1 if N0 <= N1 <= N0 + (1 << 20) else N0   # (a refused count writes nothing)
    out = (np.empty(rows + 1, dtype=np.int64), np.empty(P, dtype=np.float64), np.empty(P, dtype=np.int32),
           np.empty(P, dtype=np.int32))
    g = TgTcsr(N0, len(h[1]), *(ptr(a) for a in h))
    rc = getattr(lib, entry)(C.byref(g), N1, n, *(ptr(a) for a in new), *(ptr(a) for a in out))
    return rc, out
