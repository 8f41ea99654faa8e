"""References and cases of the T-CSR trim tests (tests/test_tcsr_trim_host.py, tests/test_hip_tcsr_trim.py).

Two references over host T-CSR arrays, every comparison exact:
  trim_numpy     per node `row[max(searchsorted(ts_row, t_cut, 'left'), len - keep_last):]` - any trim;
  trim_by_build  tg_tcsr_build_host over the events with ts >= t_cut - a horizon alone."""
import ctypes as C

import numpy as np

from _append_ref import TINY, host_build, stream

DTYPES = (np.int64, np.int64, np.float64, np.int64)


def events(s):
    return tuple(np.ascontiguousarray(a, dtype=dt) for a, dt in zip(s, DTYPES))


def trim_numpy(h, t_cut=-np.inf, keep_last=None):
    indptr, ts, nbr, eid = h
    N = len(indptr) - 1
    keep = []
    out = np.zeros(N + 1, dtype=np.int64)
    for v in range(N):
        b, e = int(indptr[v]), int(indptr[v + 1])
        s = b + int(np.searchsorted(ts[b:e], t_cut, 'left'))
        if keep_last is not None:
            s = max(s, e - keep_last)
        keep.append(np.arange(s, e, dtype=np.int64))
        out[v + 1] = out[v] + (e - s)
    idx = np.concatenate(keep) if keep else np.zeros(0, dtype=np.int64)
    return out, ts[idx], nbr[idx], eid[idx]


def trim_by_build(N, ev, t_cut):
    m = ev[2] >= t_cut
    return host_build(N, *(np.ascontiguousarray(a[m]) for a in ev))


def host_trim(h, t_cut=-np.inf, keep_last=-1):
    """tg_tcsr_trim_host on host arrays h -> (rc, arrays cut to the kept entries, kept entries)"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    N, P = len(h[0]) - 1, len(h[1])
    out = (np.full(N + 1, -7, dtype=np.int64), np.empty(P, dtype=np.float64), np.empty(P, dtype=np.int32),
           np.empty(P, dtype=np.int32))
    kept = C.c_int64(-1)
    g = TgTcsr(N, P, *(ptr(a) for a in h))
    rc = lib.tg_tcsr_trim_host(C.byref(g), float(t_cut), int(keep_last), *(ptr(a) for a in out), C.byref(kept))
    if rc != 0:
        return rc, out, kept.value
    return rc, (out[0],) + tuple(a[:kept.value] for a in out[1:]), kept.value


def max_degree(h):
    return int(np.diff(h[0]).max())


def unsorted_stream(N=50, E=300, seed=41):
    s = stream(N, E, seed=seed)
    perm = np.random.RandomState(0).permutation(E)
    return tuple(np.ascontiguousarray(a[perm]) for a in s)


def repeated_time(ev):
    """a time that occurs several times in the stream, away from its ends"""
    vals, cnt = np.unique(ev[2], return_counts=True)
    st = np.sort(ev[2])
    mid = (cnt > 2) & (vals > st[len(st) // 4]) & (vals < st[3 * len(st) // 4])
    assert mid.any()
    return float(vals[mid][0])


# a self loop is a node's last event: its two entries are the last two of the row, a cap of 1 keeps only the flag-1 entry
LOOP = (np.array([1, 2, 4, 4]), np.array([4, 4, 3, 4]), np.array([1.0, 2.0, 3.0, 5.0]), np.array([10, 11, 12, 13]))

# name -> (N, events)
STREAMS = {
    'N2-E1': (2, stream(2, 1, seed=1)),
    'tiny': (5, TINY),
    'N65-E201': (65, stream(65, 201, seed=2)),
    'N1000-E2048': (1000, stream(1000, 2048, seed=3)),
    'hub': (300, stream(300, 4000, seed=5, hub=7)),
    'N9228-E300': (9228, stream(9228, 300, seed=4)),   # mostly empty rows
    'unsorted': (50, unsorted_stream()),
    'self-loop': (6, LOOP),
}


def trims_of(name):
    """-> list of (label, t_cut, keep_last or None) for a stream: the horizon at a repeated time, below and above every
    time, the caps 0, 1 and the maximum degree, and both together"""
    N, s = STREAMS[name]
    ev = events(s)
    ts = ev[2]
    h = host_build(N, *ev)
    out = [('copy', -np.inf, None), ('below-all', float(ts.min()) - 1.0, None), ('at-first', float(ts.min()), None),
           ('above-all', float(ts.max()) + 1.0, None), ('at-last', float(ts.max()), None), ('+inf', np.inf, None),
           ('keep0', -np.inf, 0), ('keep1', -np.inf, 1), ('keep3', -np.inf, 3), ('keep-maxdeg', -np.inf, max_degree(h)),
           ('keep-huge', -np.inf, 2 ** 40)]
    if len(ts) > 100:
        t = repeated_time(ev)
        out += [('repeated-time', t, None), ('repeated-time+keep2', t, 2), ('median+keep5', float(np.median(ts)), 5)]
    else:
        out += [('mid', float(np.sort(ts)[len(ts) // 2]), None), ('mid+keep1', float(np.sort(ts)[len(ts) // 2]), 1)]
    return out
