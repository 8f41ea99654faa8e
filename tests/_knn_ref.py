"""Shared cases, references and the guarded C-ABI call of the nearest-neighbour tests (tests/test_knn_host.py,
tests/test_hip_knn.py, tests/test_hip_similar.py): tiger_hip.h: tg_knn_rows.

Two input families.
  exact: small-integer operands and power-of-two scales - every partial sum of a dot product is an integer below 2^24
    times a power of two, so float32 gives the same bits in ANY summation order and the reference is numpy int64 plus
    _topk_ref.numpy_topk, independent of the host twin.  Constructed query rows ride on fixed catalogue coordinates:
    c[j, 0] = j (q = e0: scores strictly increasing with the column, q = -e0: strictly decreasing), c[j, 1] = 1 (q = e1:
    all scores equal); the other coordinates are integers in [-8, 8].
  float: standard normal operands with NaN / +inf / -inf entries and rows of +-0.0.  At d <= 8 about 3 % of the entries are
    non-finite; above that 3 % of the ENTRIES would leave no finite pair (1 - 0.97^(2d)), so about 3 % of the rows of q and
    of c carry one non-finite entry instead.  The twin's full matrix is checked against float64, its lists against
    numpy_topk on its own bits, and the device against the twin bit for bit.
"""
import functools

import numpy as np
import torch

from _topk_ref import GUARD_F32, GUARD_I32, GUARD_I64, numpy_topk
from www2023tiger_amd import _lib
from www2023tiger_amd._lib import lib

QT, CT = _lib.TG_KNN_Q_TILE, _lib.TG_KNN_C_TILE

# (Q, C, d, k, n_split, options).  Every Q, C, d, k and n_split of the issue appears; d = 284 / 288 are the last width
# with 128 resident query rows and the first with 64; `pad`: ldq / ldc above d with NaN in the padding; `mis`: a base
# pointer 4 bytes off a 16-byte boundary (the scalar-load path); `plain`: no ids, scales, exclude or mask (NULL pointers).
SHAPES = [
    (0, 33, 4, 1, 0, ''),
    (1, 0, 8, 10, 1, ''),
    (1, 1, 28, 64, 2, 'pad'),
    (31, 31, 32, 10, 3, 'plain'),
    (32, 32, 36, 1, 0, 'mis'),
    (33, 33, 172, 10, 2, 'pad mis'),
    (QT - 1, CT - 1, 256, 64, 1, ''),
    (QT + 1, CT, 512, 10, 3, 'pad'),
    (2 * QT + 1, CT + 1, 4, 64, 5, ''),
    (33, 2 * CT + 1, 284, 10, 2, 'plain pad'),
    (65, 4097, 288, 64, 0, ''),
    (31, 4097, 8, 10, 100, 'mis'),
    (QT, 4 * CT, 32, 10, 0, 'plain'),
]
SHAPE_IDS = [f'Q{s[0]}-C{s[1]}-d{s[2]}-k{s[3]}-ns{s[4]}{"-" + s[5].replace(" ", "-") if s[5] else ""}' for s in SHAPES]


def _strided(rows, ld, mis):
    """-> (flat NaN-filled buffer, offset): rows x ld floats start at buffer[offset]; with `mis` that address is 4 bytes
    past a 16-byte boundary, without it on one"""
    buf = np.full(rows * ld + 8, np.nan, dtype=np.float32)
    want = 1 if mis else 0
    off = (want - buf.ctypes.data // 4) % 4
    return buf, off


@functools.lru_cache(maxsize=None)
def knn_case(Q, C, d, family, opts='', seed=0, mask='random', dup=False):
    """-> dict of numpy arrays: q [Q, d] / c [C, d] (views into qbuf / cbuf at qoff / coff with row strides ldq / ldc),
    ids, q_scale, c_scale, exclude, col_mask (None under `plain`).  Cached: the arrays are shared, never written."""
    rs = np.random.RandomState(seed + 7919 * Q + 104729 * C + d)
    pad, mis, plain = 'pad' in opts, 'mis' in opts, 'plain' in opts
    ldq = d + (4 if pad else 0) + (1 if mis else 0)   # `mis`: a row stride that is no multiple of 16 bytes as well
    ldc = d + (8 if pad else 0)
    qbuf, qoff = _strided(Q, ldq, mis)
    cbuf, coff = _strided(C, ldc, mis)
    q = qbuf[qoff:qoff + Q * ldq].reshape(Q, ldq)[:, :d]
    c = cbuf[coff:coff + C * ldc].reshape(C, ldc)[:, :d]
    if family == 'exact':
        q[:] = rs.randint(-8, 9, (Q, d))
        c[:] = rs.randint(-8, 9, (C, d))
        c[:, 0] = np.arange(C)
        c[:, 1] = 1
        for i in range(Q):
            kind = i % 5
            if kind in (1, 2, 3):
                q[i] = 0
                q[i, (0, 0, 1)[kind - 1]] = (1, -1, 1)[kind - 1]   # increasing, decreasing, all equal
        if dup and C > 6:
            c[5] = c[3]
            c[6] = c[3]
        q_scale = (2.0 ** rs.randint(-3, 4, Q)).astype(np.float32) * np.where(rs.rand(Q) < 0.2, -1, 1).astype(np.float32)
        c_scale = (2.0 ** rs.randint(-3, 4, C)).astype(np.float32)
        if dup and C > 6:
            c_scale[5] = c_scale[6] = c_scale[3]
    else:
        q[:] = rs.standard_normal((Q, d))
        c[:] = rs.standard_normal((C, d))
        bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        for a in (q, c):
            n = a.shape[0]
            if d <= 8:
                hit = rs.rand(n, d) < 0.03
                a[hit] = bad[rs.randint(0, 3, int(hit.sum()))]
            else:
                rows = np.nonzero(rs.rand(n) < 0.03)[0]
                a[rows, rs.randint(0, d, len(rows))] = bad[rs.randint(0, 3, len(rows))]
            zero_rows = np.nonzero(rs.rand(n) < 0.05)[0]
            a[zero_rows] = np.array([0.0, -0.0], dtype=np.float32)[rs.randint(0, 2, (len(zero_rows), d))]
        q_scale = (1.0 / np.maximum(rs.rand(Q), 0.05)).astype(np.float32)
        c_scale = (rs.standard_normal(C) / 3).astype(np.float32)    # negative ones too
        c_scale[rs.rand(C) < 0.05] = 0.0                            # a zero norm's reciprocal by convention
    ids = rs.randint(1, 1 << 40, C).astype(np.int64)
    ids[rs.rand(C) < 0.06] = 0
    if C > 8:
        ids[2], ids[4] = 111, 222
        ids[7] = ids[2]                                             # one id on two columns
    # exclude hits 0 columns (an absent id, and 0), 1 column and 2 columns
    exclude = np.array([1 << 41, 222, 111, 0], dtype=np.int64)[np.arange(Q) % 4]
    if mask == 'zero':
        col_mask = np.zeros(C, dtype=bool)
    else:
        col_mask = rs.rand(C) > 0.15
    case = dict(Q=Q, C=C, d=d, ldq=ldq, ldc=ldc, qbuf=qbuf, qoff=qoff, cbuf=cbuf, coff=coff, q=q, c=c, family=family,
                ids=None if plain else ids, q_scale=None if plain else q_scale, c_scale=None if plain else c_scale,
                exclude=None if plain else exclude, col_mask=None if plain else col_mask)
    for v in (q, c, qbuf, cbuf, ids, q_scale, c_scale, exclude, col_mask):
        v.setflags(write=False)
    return case


def _ids_and_mask(case):
    """the ids of the columns and the [Q, C] mask that tg_topk_rows would be given"""
    Q, C = case['Q'], case['C']
    ids = np.arange(1, C + 1, dtype=np.int64) if case['ids'] is None else case['ids']
    mask = np.ones((Q, C), dtype=bool)
    if case['col_mask'] is not None:
        mask &= case['col_mask'][None, :]
    if case['exclude'] is not None:
        mask &= ids[None, :] != case['exclude'][:, None]
    return ids, mask


def exact_scores(case):
    """float32 [Q, C] of an exact-family case from int64 arithmetic (the products with the power-of-two scales are exact)"""
    assert case['family'] == 'exact'
    s = (case['q'].astype(np.int64) @ case['c'].astype(np.int64).T).astype(np.float64)
    assert np.abs(s).max(initial=0) < 2 ** 24
    if case['q_scale'] is not None:
        s = s * case['q_scale'].astype(np.float64)[:, None]
    if case['c_scale'] is not None:
        s = s * case['c_scale'].astype(np.float64)[None, :]
    out = s.astype(np.float32)
    assert (out.astype(np.float64) == s).all()
    return out


def reference_topk(case, scores, k):
    """numpy_topk on a [Q, C] float32 matrix with the case's ids, mask and exclusions"""
    ids, mask = _ids_and_mask(case)
    return numpy_topk(scores, ids, k, mask)


def float64_scores(case):
    """(S64 [Q, C], bound [Q, C], finite [Q, C]): the float64 scores, the fma-chain bound d 2^-24 sum|q c| times the scales,
    and which pairs have only finite operands"""
    q64, c64 = case['q'].astype(np.float64), case['c'].astype(np.float64)
    finq, finc = np.isfinite(q64).all(1), np.isfinite(c64).all(1)
    qz, cz = np.where(np.isfinite(q64), q64, 0.0), np.where(np.isfinite(c64), c64, 0.0)
    s = qz @ cz.T
    mag = np.abs(qz) @ np.abs(cz).T
    for sc, axis in ((case['q_scale'], 0), (case['c_scale'], 1)):
        if sc is not None:
            sc = sc.astype(np.float64)[:, None] if axis == 0 else sc.astype(np.float64)[None, :]
            s, mag = s * sc, mag * np.abs(sc)
    return s, case['d'] * 2.0 ** -24 * mag, finq[:, None] & finc[None, :]


def _dev(x, device):
    return None if x is None else torch.tensor(np.asarray(x)).to(device)


def case_tensors(case, device):
    """torch views with the case's strides and base offsets on `device` (bool mask as uint8)"""
    Q, C, d = case['Q'], case['C'], case['d']
    qb, cb = _dev(case['qbuf'], device), _dev(case['cbuf'], device)
    q = qb[case['qoff']:case['qoff'] + Q * case['ldq']].view(Q, case['ldq'])[:, :d]
    c = cb[case['coff']:case['coff'] + C * case['ldc']].view(C, case['ldc'])[:, :d]
    mask = None if case['col_mask'] is None else _dev(case['col_mask'].astype(np.uint8), device)
    return dict(q=q, c=c, ids=_dev(case['ids'], device), q_scale=_dev(case['q_scale'], device),
                c_scale=_dev(case['c_scale'], device), exclude=_dev(case['exclude'], device), col_mask=mask)


def run_knn(case, k, n_split, device='cpu', want_matrix=False, ws_short=0):
    """Calls tg_knn_rows_host (device 'cpu') or tg_knn_rows through the C ABI with outputs of Q + 2 rows pre-filled with the
    guards of _topk_ref; asserts the two rows past Q untouched.  -> (rc, dict of numpy results [, the twin's matrix])"""
    from www2023tiger_amd.hip_ops import stream_ptr
    Q, C, d = case['Q'], case['C'], case['d']
    t = case_tensors(case, device)
    p = lambda x: None if x is None else x.data_ptr()
    out = dict(ids=torch.full((Q + 2, k), int(GUARD_I64), dtype=torch.int64, device=device),
               scores=torch.full((Q + 2, k), float(GUARD_F32), dtype=torch.float32, device=device),
               cols=torch.full((Q + 2, k), int(GUARD_I32), dtype=torch.int32, device=device),
               n_valid=torch.full((Q + 2,), int(GUARD_I32), dtype=torch.int32, device=device),
               n_nonfinite=torch.zeros(1, dtype=torch.int64, device=device))
    args = (Q, C, d, k, p(t['q']) if Q else None, case['ldq'], p(t['c']) if C else None, case['ldc'], p(t['ids']),
            p(t['q_scale']), p(t['c_scale']), p(t['exclude']), p(t['col_mask']), n_split, p(out['ids']), p(out['scores']),
            p(out['cols']), p(out['n_valid']), p(out['n_nonfinite']))
    matrix = None
    if device == 'cpu':
        matrix = torch.full((Q, C), float(GUARD_F32), dtype=torch.float32) if want_matrix else None
        rc = lib.tg_knn_rows_host(*args, p(matrix))
    else:
        nbytes = int(lib.tg_knn_rows_workspace_bytes(Q, C, k, n_split)) - ws_short
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        rc = lib.tg_knn_rows(*args, ws.data_ptr(), max(nbytes, 0), stream_ptr(torch.device(device)))
        torch.cuda.synchronize()
    res = {key: v.cpu().numpy() for key, v in out.items()}
    for key, guard in (('ids', GUARD_I64), ('scores', GUARD_F32), ('cols', GUARD_I32), ('n_valid', GUARD_I32)):
        assert (res[key][Q:] == guard).all(), f'{key}: rows past Q were written'
        res[key + '_all'] = res[key]
        res[key] = res[key][:Q]
    if want_matrix:
        return rc, res, matrix.numpy()
    return rc, res


def untouched(res):
    """every output still holds its guard (a refusal wrote nothing)"""
    return all((res[key + '_all'] == guard).all() for key, guard in
               (('ids', GUARD_I64), ('scores', GUARD_F32), ('cols', GUARD_I32), ('n_valid', GUARD_I32))) \
        and int(res['n_nonfinite'][0]) == 0


@functools.lru_cache(maxsize=None)
def twin_topk(Q, C, d, k, family, opts='', mask='random', dup=False):
    """the host twin's result for a case (computed once, shared by the device tests; read-only)"""
    rc, res = run_knn(knn_case(Q, C, d, family, opts, mask=mask, dup=dup), k, 0, 'cpu')
    assert rc == _lib.TG_OK
    res = {key: res[key] for key in ('ids', 'scores', 'cols', 'n_valid')} | {'n_nonfinite': int(res['n_nonfinite'][0])}
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res
