"""Numpy references and shared inputs of the top-k tests (tests/test_topk_host.py, tests/test_hip_topk.py,
tests/test_hip_recommend.py): np.lexsort on (column, -score) after the leave-out rules of tiger_hip.h: tg_topk_rows, and a
plain loop over the events for the seen mask."""
import numpy as np

GUARD_I64 = np.int64(-0x0123456789ABCDEF)
GUARD_I32 = np.int32(-0x01234567)
GUARD_F32 = np.float32(-12345.678)


def numpy_topk(scores, cand, k, mask=None):
    """-> dict(ids int64 [B, k], scores float32 [B, k], cols int32 [B, k], n_valid int32 [B], n_nonfinite int).
    scores [B, C] float32; cand [B, C] or [C]; mask bool [B, C] or None.  Left out: id 0, mask false, non-finite score
    (counted when the first two rules left it in).  Order: score descending, equal scores by ascending column."""
    scores = np.asarray(scores)
    B, C = scores.shape
    ids_all = np.broadcast_to(np.asarray(cand), (B, C))
    left = ids_all != 0
    if mask is not None:
        left = left & np.asarray(mask).astype(bool)
    fin = np.isfinite(scores)
    out = dict(ids=np.zeros((B, k), np.int64), scores=np.full((B, k), -np.inf, np.float32), cols=np.full((B, k), -1, np.int32),
               n_valid=np.zeros(B, np.int32), n_nonfinite=int((left & ~fin).sum()))
    for i in range(B):
        cols = np.nonzero(left[i] & fin[i])[0]
        s = scores[i, cols]
        order = cols[np.lexsort((cols, -s))][:k]   # last key first: -score, then the column (-0.0 == +0.0 for '<')
        n = len(order)
        out['ids'][i, :n] = ids_all[i, order]
        out['scores'][i, :n] = scores[i, order]
        out['cols'][i, :n] = order
        out['n_valid'][i] = len(cols)
    return out


def assert_same_topk(got, want, what=''):
    """ids, cols, n_valid, the score BITS and the non-finite count: exactly"""
    for key in ('ids', 'cols', 'n_valid'):
        np.testing.assert_array_equal(np.asarray(got[key]), want[key], err_msg=f'{what} {key}')
    np.testing.assert_array_equal(np.asarray(got['scores']).view(np.uint32), want['scores'].view(np.uint32),
                                  err_msg=f'{what} score bits')
    assert int(np.asarray(got['n_nonfinite']).reshape(-1)[0]) == want['n_nonfinite'], what


ROW_KINDS = ('normal', 'quant4', 'all_equal', 'zeros', 'all_masked', 'all_nonfinite')


def topk_case(B, C, *, shared, with_mask, ld=None, seed=0, first_kind=0):
    """scores (a [B, C] view of a NaN-filled [B, ld] array), cand ([C] or [B, C], id 0 scattered), mask (bool or None).
    Row i is of kind ROW_KINDS[(first_kind + i) % 6]: normal scores; scores quantised to 4 values (mostly ties); one value
    in every column; +0.0 / -0.0 / +-1 mixed; every column left out; every score non-finite.  On top, about 4 % of all
    entries are NaN / +inf / -inf wherever they fall: in columns left in (counted) and in left-out ones (not counted)."""
    rs = np.random.RandomState(seed + 1000 * B + C)
    ld = C if ld is None else ld
    full = np.full((B, ld), np.nan, dtype=np.float32)
    s = full[:, :C]
    cand = rs.randint(1, 1 << 40, size=(C,) if shared else (B, C)).astype(np.int64)
    cand[rs.rand(*cand.shape) < 0.06] = 0
    if not shared and C > 3:
        cand[:, 2] = cand[:, 1]   # a duplicate id is two columns
    mask = rs.rand(B, C) > 0.2 if with_mask else None
    for i in range(B):
        kind = ROW_KINDS[(first_kind + i) % len(ROW_KINDS)]
        if kind == 'normal':
            s[i] = rs.standard_normal(C)
        elif kind == 'quant4':
            s[i] = rs.randint(0, 4, C) * 0.5 - 0.75
        elif kind == 'all_equal':
            s[i] = 0.375
        elif kind == 'zeros':
            s[i] = np.array([0.0, -0.0, 1.0, -1.0, -0.0, 0.0], dtype=np.float32)[rs.randint(0, 6, C)]
        elif kind == 'all_masked':
            s[i] = rs.standard_normal(C)
            if mask is not None:
                mask[i] = False
            elif not shared:
                cand[i] = 0
        else:
            s[i] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[np.arange(C) % 3]
    bad = rs.rand(B, C) < 0.04
    s[bad] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[rs.randint(0, 3, int(bad.sum()))]
    return s, cand, mask


# ---- seen mask ---------------------------------------------------------------------------------------------------------
def seen_graph():
    """About 40 nodes.  Sources 1..4 have 63, 64, 65 and 200 entries (they are never a destination), node 5 has none; the
    destinations are 10..40, so neighbours repeat; event times come in equal pairs.  -> (src, dst, ts, n_nodes)"""
    rs = np.random.RandomState(7)
    src, dst, ts = [], [], []
    for s, deg in ((1, 63), (2, 64), (3, 65), (4, 200)):
        src += [s] * deg
        dst += rs.randint(10, 41, deg).tolist()
        ts += [float(j // 2 + 1) for j in range(deg)]
    order = np.argsort(np.asarray(ts), kind='stable')
    return (np.asarray(src, np.int64)[order], np.asarray(dst, np.int64)[order], np.asarray(ts, np.float64)[order], 41)


def seen_queries():
    """(src, ts, catalogue): every source before anything, at an entry's own time (strict: that entry does not count), in
    the middle, after everything; destinations as sources (their neighbours 1..4 are mostly outside the catalogue); the
    node without entries.  The catalogue leaves 35..40 out and holds source 2."""
    q = []
    for s, deg in ((1, 63), (2, 64), (3, 65), (4, 200)):
        last = float((deg - 1) // 2 + 1)
        q += [(s, 0.0), (s, 1.0), (s, 2.0), (s, last / 2), (s, last), (s, last + 1.0), (s, 1.5)]
    q += [(5, 1000.0), (10, 1000.0), (17, 5.0), (40, 1000.0), (36, 3.0)]
    src = np.asarray([a for a, _ in q], np.int64)
    ts = np.asarray([b for _, b in q], np.float64)
    cat = np.random.RandomState(3).permutation(np.concatenate([np.arange(10, 35), [2]])).astype(np.int64)
    return src, ts, cat


def numpy_seen_mask(ev_src, ev_dst, ev_ts, src, ts, cat, mask=None):
    """bool [B, C]: the caller's mask (default: all true) with column c cleared where cat[c] is the other endpoint of an
    event of src[i] - in either direction - strictly before ts[i]"""
    B, C = len(src), len(cat)
    out = np.ones((B, C), dtype=bool) if mask is None else np.array(mask, dtype=bool)
    col = {int(n): c for c, n in enumerate(cat)}
    for i in range(B):
        for u, v, t in zip(ev_src, ev_dst, ev_ts):
            if not t < ts[i]:
                continue
            for a, b in ((u, v), (v, u)):
                if a == src[i] and int(b) in col:
                    out[i, col[int(b)]] = False
    return out
