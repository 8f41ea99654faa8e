"""References and cases of the T-CSR erase tests (tests/test_tcsr_erase_host.py, tests/test_hip_tcsr_erase.py).

Two references over host T-CSR arrays, every comparison exact:
  erase_numpy     the owner of every entry by np.repeat, one boolean mask over the entries - any erase;
  erase_by_build  tg_tcsr_build_host over the events with src, dst not in S and eid not in R."""
import ctypes as C

import numpy as np

from _append_ref import host_build


def bitmap(ids, n):
    """what new_bitmap + bitmap_mark give over n ids, as a numpy int64 array (ids at or beyond n are not marked)"""
    bits = np.zeros((n + 63) // 64, dtype=np.uint64)
    for i in np.unique(np.asarray(ids, dtype=np.int64)):
        if 0 <= i < n:
            bits[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return bits.view(np.int64)


def keep_mask(h, S=None, R=None, n_rows=None):
    """bool per entry: kept.  S: erased node ids or None, R: retracted eids or None, n_rows: the ids the eid bitmap covers
    (default 1 + max(R)); an eid at or beyond it is never matched."""
    indptr, ts, nbr, eid = h
    owner = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    keep = np.ones(len(ts), dtype=bool)
    if S is not None:
        S = np.asarray(S, dtype=np.int64)
        keep &= ~np.isin(owner, S) & ~np.isin(nbr.astype(np.int64), S)
    if R is not None:
        R = np.asarray(R, dtype=np.int64)
        if n_rows is None:
            n_rows = int(R.max()) + 1 if len(R) else 0
        keep &= ~np.isin((eid.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64), R[R < n_rows])
    return keep, owner


def erase_numpy(h, S=None, R=None, n_rows=None):
    keep, owner = keep_mask(h, S, R, n_rows)
    N = len(h[0]) - 1
    indptr = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=N))]).astype(np.int64)
    return indptr, h[1][keep], h[2][keep], h[3][keep]


def filtered(ev, S=None, R=None):
    """the events with src, dst not in S and eid not in R"""
    m = np.ones(len(ev[0]), dtype=bool)
    if S is not None:
        m &= ~np.isin(ev[0], S) & ~np.isin(ev[1], S)
    if R is not None:
        m &= ~np.isin(ev[3], R)
    return tuple(np.ascontiguousarray(a[m]) for a in ev)


def erase_by_build(N, ev, S=None, R=None):
    return host_build(N, *filtered(ev, S, R))


def host_erase(h, S=None, R=None, n_rows=None):
    """tg_tcsr_erase_host on host arrays h -> (rc, arrays cut to the kept entries, kept entries)"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    N, P = len(h[0]) - 1, len(h[1])
    if R is not None and n_rows is None:
        n_rows = int(np.max(R)) + 1 if len(R) else 0
    nb = None if S is None else bitmap(S, N)
    eb = None if R is None else bitmap(R, n_rows)
    out = (np.full(N + 1, -7, dtype=np.int64), np.empty(P, dtype=np.float64), np.empty(P, dtype=np.int32),
           np.empty(P, dtype=np.int32))
    kept = C.c_int64(-1)
    g = TgTcsr(N, P, *(ptr(a) for a in h))
    rc = lib.tg_tcsr_erase_host(C.byref(g), ptr(nb), ptr(eb), 0 if n_rows is None else int(n_rows), *(ptr(a) for a in out),
                                C.byref(kept))
    if rc != 0:
        return rc, out, kept.value
    return rc, (out[0],) + tuple(a[:kept.value] for a in out[1:]), kept.value


def small_eids(ev):
    """the stream with eids 1 .. E in order (a bitmap over arbitrary 31-bit eids would take 256 MiB)"""
    return ev[0], ev[1], ev[2], np.arange(1, len(ev[0]) + 1, dtype=np.int64)
