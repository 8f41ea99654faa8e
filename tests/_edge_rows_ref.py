"""Reference and cases of the edge-row release tests (tests/test_edge_rows_host.py, tests/test_hip_edge_rows.py,
tests/test_hip_release_rows.py).  Every comparison is exact: integers and bit patterns.

  release_numpy  live = unique(eid & 0x7FFFFFFF) U {0} U pin U [keep_from, n_rows); remap by cumsum; the table by fancy
                 indexing; the eids by a gather, bit 31 carried over.
The kernels read nothing of a graph but its eid array, so most cases are an eid array and a row count."""
import ctypes as C

import numpy as np

from _append_ref import TINY, host_build, stream

GUARD32 = -0x5A5A5A5B   # what untouched int32 outputs hold


def release_numpy(eid, table, n_rows, keep_from=None, pin=None):
    """-> (remap int32 [n_rows], table_out or None, eid_out int32)"""
    keep_from = n_rows if keep_from is None else keep_from
    e = np.asarray(eid).view(np.uint32)
    live = np.unique(np.concatenate([(e & np.uint32(0x7FFFFFFF)).astype(np.int64), [0],
                                     np.asarray([] if pin is None else pin, dtype=np.int64).reshape(-1),
                                     np.arange(keep_from, n_rows, dtype=np.int64)]))
    assert live.min() >= 0 and live.max() < n_rows
    mark = np.zeros(n_rows, dtype=np.int64)
    mark[live] = 1
    remap = np.where(mark == 1, np.cumsum(mark) - 1, -1).astype(np.int32)
    eid_out = (remap[e & np.uint32(0x7FFFFFFF)].view(np.uint32) | (e & np.uint32(0x80000000))).view(np.int32)
    return remap, (None if table is None else table[live]), eid_out


def host_release(eid, table, n_rows, keep_from=None, pin=None):
    """tg_edge_rows_host on an eid array -> (rc, remap, table_out cut to the live rows, eid_out, n_live); the outputs are
    pre-filled, so an untouched one shows"""
    from www2023tiger_amd._lib import TgTcsr, lib, ptr
    eid = np.ascontiguousarray(eid, dtype=np.int32)
    g = TgTcsr(1, len(eid), None, None, None, ptr(eid) if len(eid) else None)
    p = None if pin is None else np.ascontiguousarray(pin, dtype=np.int64)
    remap = np.full(n_rows, GUARD32, dtype=np.int32)
    eid_out = np.full(len(eid), GUARD32, dtype=np.int32)
    t_out = None if table is None else np.full(table.shape, GUARD32, dtype=np.int32).view(np.float32)
    n_live = C.c_int64(-7)
    rc = lib.tg_edge_rows_host(C.byref(g), ptr(table), n_rows, 0 if table is None else table.shape[1],
                               n_rows if keep_from is None else keep_from, ptr(p), 0 if p is None else len(p), ptr(remap),
                               ptr(t_out), ptr(eid_out), C.byref(n_live))
    if rc == 0 and t_out is not None:
        assert (t_out[n_live.value:].view(np.int32) == GUARD32).all(), 'rows behind the live ones were written'
        t_out = t_out[:n_live.value]
    return rc, remap, t_out, eid_out, n_live.value


def table_of(n_rows, d_e, seed=0, special=False):
    """float32 [n_rows, d_e]; special: NaNs with payloads, infinities, denormals and -0.0 among the values"""
    rs = np.random.RandomState(seed)
    t = rs.standard_normal((n_rows, d_e)).astype(np.float32)
    if special:
        bits = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000, 0x7F800001],
                        dtype=np.uint32).view(np.float32)
        m = rs.uniform(size=t.shape) < 0.5
        t[m] = bits[rs.randint(0, len(bits), int(m.sum()))]
    return t


def flagged(rows, seed=0):
    """row ids -> an eid array with a random direction flag in bit 31"""
    rows = np.asarray(rows, dtype=np.int64)
    f = np.random.RandomState(seed).randint(0, 2, len(rows)).astype(np.uint32) << np.uint32(31)
    return (rows.astype(np.uint32) | f).view(np.int32)


def row_stream(N, E, seed=0, **kw):
    """the events of _append_ref.stream with eids 1 .. E: the rows of a table of E + 1 rows, row 0 the padding row"""
    s = stream(N, E, seed=seed, **kw)
    return (np.ascontiguousarray(s[0], dtype=np.int64), np.ascontiguousarray(s[1], dtype=np.int64),
            np.ascontiguousarray(s[2], dtype=np.float64), np.arange(1, E + 1, dtype=np.int64))


def tiny_eids():
    t = [np.ascontiguousarray(a) for a in TINY]
    E = len(t[0])
    return host_build(5, t[0].astype(np.int64), t[1].astype(np.int64), t[2].astype(np.float64),
                      np.arange(1, E + 1, dtype=np.int64))[3], E + 1


def patterns(n):
    """name -> eid array over a table of n rows (n >= 4)"""
    rs = np.random.RandomState(n)
    return {
        'all-live': flagged(rs.permutation(np.arange(1, n)), 1),
        'none-but-0': np.zeros(0, dtype=np.int32),
        'last-only': flagged([n - 1], 2),
        'alternating': flagged(np.arange(1, n, 2), 3),
        'self-loop': np.array([n // 2, n // 2 | -0x80000000], dtype=np.int64).astype(np.int32),   # one eid, both flags
        'multi-edges': flagged(np.repeat(rs.randint(1, n, max(n // 8, 2)), 3), 4),
        'random-third': flagged(rs.randint(0, n, n // 3), 5),
    }
