"""Reference and cases of the T-CSR verifier tests (tests/test_tcsr_verify_host.py, tests/test_hip_tcsr_verify.py).

verify_numpy: the six classes and the maximum time over host T-CSR arrays, with numpy's vector operations and
searchsorted - written from the contract in tiger_hip.h, not from the host twin (which walks row by row).  Every
comparison is exact."""
import ctypes as C

import numpy as np

from _append_ref import TINY, host_build, stream

ENDS, PTR_ORDER, TS_ORDER, TS_NAN, NBR_RANGE, EID_RANGE = 1, 2, 4, 8, 16, 32
DTYPES = (np.int64, np.int64, np.float64, np.int64)


def _first(mask):
    hit = np.flatnonzero(mask)
    return int(hit[0]) if len(hit) else -1


def verify_numpy(h, eid_rows=-1):
    """-> (code, first[6], t_max)"""
    indptr, ts, nbr, eid = h
    N, P = len(indptr) - 1, len(ts)
    first = [-1] * 6
    if indptr[0] != 0:
        first[0] = 0
    elif indptr[N] != P:
        first[0] = N
    first[1] = _first(indptr[1:] < indptr[:-1])
    nan = np.isnan(ts)
    first[3] = _first(nan)
    first[4] = _first((nbr < 0) | (nbr.astype(np.int64) >= N))
    if eid_rows >= 0:
        first[5] = _first((eid.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64) >= eid_rows)
    if first[0] < 0 and first[1] < 0 and P > 1:
        # owner(p) = (first v in [1, N) with indptr[v] > p, else N) - 1 = how many of indptr[1 .. N - 1] are <= p
        owner = np.searchsorted(indptr[1:N], np.arange(P, dtype=np.int64), side='right')
        with np.errstate(invalid='ignore'):
            down = ts[1:] < ts[:-1]   # (False for a NaN on either side)
        hit = _first(down & (owner[1:] == owner[:-1]))
        first[2] = hit + 1 if hit >= 0 else -1
    code = sum(1 << c for c in range(6) if first[c] >= 0)
    good = ts[~nan]
    t_max = float(good.max()) if len(good) else -np.inf
    if t_max == 0.0:
        t_max = 0.0 if np.any((good == 0.0) & ~np.signbit(good)) else -0.0
    return code, first, t_max


def same_result(got, want, what=''):
    assert got[0] == want[0] and list(got[1]) == list(want[1]), f'{what}: {got} against {want}'
    a, b = np.float64(got[2]), np.float64(want[2])
    assert a.view(np.int64) == b.view(np.int64), f'{what}: t_max {got[2]!r} against {want[2]!r}'


def host_verify(h, eid_rows=-1):
    """tg_tcsr_verify_host on host arrays h -> (rc, (code, first, t_max))"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    out8 = np.full(8, -77, dtype=np.int64)
    g = TgTcsr(len(h[0]) - 1, len(h[1]), *(ptr(a) for a in h))
    rc = lib.tg_tcsr_verify_host(C.byref(g), int(eid_rows), ptr(out8))
    return rc, (int(out8[0]), [int(x) for x in out8[1:7]], float(out8[7:8].view(np.float64)[0]))


def events(N, E, seed):
    """time-ordered events over [0, N) with multi-edges and self loops and eids 1 .. E -> typed arrays"""
    s = stream(N, E, seed=seed)
    s = (s[0], s[1], s[2], np.arange(1, E + 1))
    return tuple(np.ascontiguousarray(a, dtype=dt) for a, dt in zip(s, DTYPES))


TINY_EV = tuple(np.ascontiguousarray(a, dtype=dt) for a, dt in zip(TINY, DTYPES))
# name -> (N, events, rows of an edge table that holds every eid)
CLEAN = {
    'tiny': (5, TINY_EV, 4),
    'N1-E0': (1, events(1, 0, 1), 1),
    'N2-E1': (2, events(2, 1, 2), 2),
    'N65-E200': (65, events(65, 200, 3), 201),
    'N9228-E5000': (9228, events(9228, 5000, 4), 5001),
}


def clean(name):
    N, ev, rows = CLEAN[name]
    return N, ev, rows, host_build(N, *ev)


def changed(h, which, index, value):
    """a copy of the arrays h with ONE word changed: h[which][index] = value"""
    out = [a.copy() for a in h]
    out[which][index] = value
    return tuple(out)


def inner_entry(h, nth=0):
    """the nth entry p that is no row start and sits in a row of at least 3 entries, with its row (b, e) - or None"""
    indptr = h[0]
    rows = np.flatnonzero(np.diff(indptr) >= 3)
    if len(rows) <= nth:
        return None
    v = int(rows[nth])
    return int(indptr[v]) + 1, int(indptr[v]), int(indptr[v + 1])


def one_word_cases(h, rows):
    """-> list of (label, arrays, eid_rows, the class the change must raise - 0: none, the change is legal)"""
    indptr, ts, nbr, eid = h
    N, P = len(indptr) - 1, len(ts)
    out = [('indptr[0]=1', changed(h, 0, 0, 1), rows, ENDS),
           ('indptr[N]+1', changed(h, 0, N, P + 1), rows, ENDS),
           ('indptr[N]-1', changed(h, 0, N, P - 1), rows, ENDS)]
    for label, v in (('v=0', 0), ('v=mid', N // 2), ('v=N-1', N - 1)):
        # a decreasing pair (v, v + 1): indptr[v + 1] = indptr[v] - 1  (v + 1 == N changes the end as well)
        out.append((f'decreasing pair {label}', changed(h, 0, v + 1, int(indptr[v]) - 1), rows, PTR_ORDER))
    if P:
        mid = P // 2
        out += [('nan', changed(h, 1, mid, np.nan), rows, TS_NAN),
                ('nbr=N', changed(h, 2, mid, N), rows, NBR_RANGE),
                ('nbr=-1', changed(h, 2, P - 1, -1), rows, NBR_RANGE),
                ('eid=rows', changed(h, 3, mid, rows), rows, EID_RANGE),
                ('eid=rows|flag', changed(h, 3, 0, (rows | 0x80000000) - (1 << 32)), rows, EID_RANGE),
                ('eid=rows, class off', changed(h, 3, mid, rows), -1, 0)]
        inner = inner_entry(h)
        if inner is not None:
            p, b, e = inner
            out.append(('time decrease inside a row', changed(h, 1, p, float(ts[p - 1]) - 1.0), rows, TS_ORDER))
        starts = indptr[1:N][(indptr[1:N] > 0) & (indptr[1:N] < P)]
        if len(starts):
            p = int(starts[len(starts) // 2])   # a row start: the same decrease across a row boundary is legal
            low = min(float(ts[p - 1]), float(ts[p])) - 1.0   # below the entry in front, and no later than it was
            out.append(('time decrease across a row boundary', changed(h, 1, p, low), rows, 0))
    return out


def synthetic(indptr, rows=1000, seed=0):
    """a clean T-CSR over the given row bounds: ascending times with duplicates inside every row (rows start anywhere, so
    most row starts go DOWN in time), random neighbours and eids below `rows` with random direction flags"""
    rs = np.random.RandomState(seed)
    indptr = np.asarray(indptr, dtype=np.int64)
    N, P = len(indptr) - 1, int(indptr[-1])
    ts = np.floor(rs.uniform(0, 50, P))
    for v in range(N):
        b, e = int(indptr[v]), int(indptr[v + 1])
        if e - b > 1:
            ts[b:e] = np.sort(ts[b:e])
    nbr = rs.randint(0, N, P).astype(np.int32)
    eid = (rs.randint(0, rows, P).astype(np.uint32) | (rs.randint(0, 2, P).astype(np.uint32) << np.uint32(31))).view(np.int32)
    return indptr, ts, nbr, eid


def random_rows(N, P, seed=0):
    """row bounds of N rows over P entries, cut at random (empty rows included)"""
    rs = np.random.RandomState(seed)
    cuts = np.sort(rs.randint(0, P + 1, N - 1)) if N > 1 else np.zeros(0, dtype=np.int64)
    return np.concatenate([[0], cuts, [P]]).astype(np.int64)
