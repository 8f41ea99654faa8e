"""Top-k selection and the seen mask without a GPU: the host twins tg_topk_rows_host / tg_seen_mask_host (the same keys and
the same search as the device entries) against the numpy references of tests/_topk_ref.py - exactly: ids, columns,
n_valid, score bits, mask bytes.  Argument errors of both entries of either pair, and catalogue_index."""
import ctypes

import numpy as np
import pytest
import torch

from _topk_ref import (assert_same_topk, numpy_seen_mask, numpy_topk, seen_graph, seen_queries, topk_case)

t = torch.from_numpy


def host_topk(s, cand, k, mask, n_seg=0):
    from www2023tiger_amd import hip_ops
    out = hip_ops.topk_rows(t(s), t(cand), k, mask=None if mask is None else t(mask), n_seg=n_seg)
    return {key: v.numpy() for key, v in out.items()}


@pytest.mark.parametrize('shared,with_mask', [(True, True), (False, True), (False, False)],
                         ids=['shared-masked', 'per-row-masked', 'per-row'])
@pytest.mark.parametrize('B,C', [(1, 1), (3, 63), (7, 64), (6, 65), (13, 129), (6, 1000)])
def test_host_twin_equals_numpy(B, C, shared, with_mask):
    s, cand, mask = topk_case(B, C, shared=shared, with_mask=with_mask, ld=C + 5)
    assert s.strides[0] == 4 * (C + 5)
    for k in (1, 10, 63, 64):   # k > C and k > n_valid included
        want = numpy_topk(s, cand, k, mask)
        assert_same_topk(host_topk(s, cand, k, mask), want, f'k={k}')
        assert_same_topk(host_topk(s, cand, k, mask, n_seg=7), want, f'k={k} n_seg=7')
    if B >= 6:   # every row kind is present and says what it was made to say
        assert want['n_valid'][4] == 0 and want['n_valid'][5] == 0 and (want['cols'][4] == -1).all()
        assert want['n_nonfinite'] > 0 and want['n_valid'].max() > 0


def test_order_and_padding_on_a_hand_made_row():
    """ties by ascending column, -0.0 == +0.0 with the stored bits kept, left-out columns, padding past n_valid"""
    s = np.array([[0.5, -0.0, 0.5, 0.0, np.nan, 9.0, np.inf, 0.5, -1.0, 7.0]], dtype=np.float32)
    cand = np.array([11, 12, 13, 14, 15, 0, 17, 18, 19, 20], dtype=np.int64)
    mask = np.ones((1, 10), dtype=bool)
    mask[0, 9] = False   # 7.0 is masked, 9.0 has the padding id; NaN and +inf are left in by both rules: counted
    got = host_topk(s, cand, 8, mask)
    assert got['cols'].tolist() == [[0, 2, 7, 1, 3, 8, -1, -1]]
    assert got['ids'].tolist() == [[11, 13, 18, 12, 14, 19, 0, 0]]
    assert got['n_valid'].tolist() == [6] and int(got['n_nonfinite'][0]) == 2
    assert np.signbit(got['scores'][0, 3]) and not np.signbit(got['scores'][0, 4])
    assert np.isneginf(got['scores'][0, 6:]).all()
    assert_same_topk(got, numpy_topk(s, cand, 8, mask))


def test_the_nonfinite_counter_accumulates_over_calls():
    from www2023tiger_amd import hip_ops
    s, cand, mask = topk_case(6, 65, shared=True, with_mask=True)
    want = numpy_topk(s, cand, 10, mask)
    acc = torch.zeros(1, dtype=torch.int64)
    a = hip_ops.topk_rows(t(s[:2]), t(cand), 10, mask=t(mask[:2]), acc=acc)
    b = hip_ops.topk_rows(t(s[2:]), t(cand), 10, mask=t(mask[2:]), acc=acc)
    assert a['n_nonfinite'] is acc and b['n_nonfinite'] is acc and int(acc) == want['n_nonfinite'] > 0
    np.testing.assert_array_equal(torch.cat([a['ids'], b['ids']]).numpy(), want['ids'])


def test_topk_entry_points_refuse_bad_arguments():
    from www2023tiger_amd import _lib
    lib, p = _lib.lib, _lib.ptr
    buf = np.zeros(4096, dtype=np.int64)
    o = [p(buf)] * 5
    host = lambda B, C, k, ld, n_seg=0: lib.tg_topk_rows_host(B, C, k, p(buf), ld, p(buf), 1, None, n_seg, *o)
    devc = lambda B, C, k, ld, n_seg=0, ws=None, nb=0: lib.tg_topk_rows(B, C, k, p(buf), ld, p(buf), 1, None, n_seg, *o, ws, nb, None)
    for f in (host, devc):   # (the device entry returns before it would touch a pointer)
        assert f(2, 8, 0, 8) == _lib.TG_EINVAL
        assert f(2, 8, _lib.TG_TOPK_MAX_K + 1, 8) == _lib.TG_EINVAL
        assert f(-1, 8, 4, 8) == _lib.TG_EINVAL
        assert f(2, -1, 4, 8) == _lib.TG_EINVAL
        assert f(2, 8, 4, 7) == _lib.TG_EINVAL          # ld < C
        assert f(2, 8, 4, 8, -1) == _lib.TG_EINVAL
        assert f(0, 8, 4, 8) == _lib.TG_OK              # no rows: nothing to do
    ids, sc, cols = np.ones((2, 4), np.int64), np.ones((2, 4), np.float32), np.ones((2, 4), np.int32)
    nv, bad = np.ones(2, np.int32), np.zeros(1, np.int64)
    assert lib.tg_topk_rows_host(2, 0, 4, None, 0, None, 1, None, 0, p(ids), p(sc), p(cols), p(nv), p(bad)) == _lib.TG_OK
    assert (ids == 0).all() and np.isneginf(sc).all() and (cols == -1).all() and (nv == 0).all() and bad[0] == 0  # all padding
    assert lib.tg_topk_rows_host(2, 8, 4, None, 8, None, 1, None, 0, *o) == _lib.TG_EINVAL
    assert lib.tg_topk_rows(2, 8, 4, None, 8, None, 1, None, 0, *o, None, 0, None) == _lib.TG_EINVAL
    # the workspace: nothing for one segment per row, B * n_seg * (8 k + 8) bytes otherwise; a short one is refused
    assert lib.tg_topk_rows_workspace_bytes(2, 8, 4, 1) == 0
    assert lib.tg_topk_rows_workspace_bytes(2, 8, 4, 3) == 2 * 3 * (8 * 4 + 8)
    assert lib.tg_topk_rows_workspace_bytes(2, 8, 0, 3) == 0
    assert devc(2, 8, 4, 8, 3, None, 0) == _lib.TG_EWORKSPACE
    assert devc(2, 8, 4, 8, 3, p(buf), 2 * 3 * (8 * 4 + 8) - 1) == _lib.TG_EWORKSPACE
    # the library's own choice: one segment for many short rows, several for a few long ones, and it never exceeds the
    # bytes of sqrt(C / k) segments
    assert lib.tg_topk_rows_workspace_bytes(4096, 1000, 10, 0) == 0
    n = lib.tg_topk_rows_workspace_bytes(1, 1 << 20, 64, 0) // (8 * 64 + 8)
    assert 2 <= n <= 128


def test_symbols_resolve_and_the_abi_version_stays():
    from www2023tiger_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('tg_topk_rows', 'tg_topk_rows_host', 'tg_topk_rows_workspace_bytes', 'tg_seen_mask', 'tg_seen_mask_host'):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.lib.tg_abi_version() == 9 and _lib.TG_TOPK_MAX_K == 64


def test_python_surface_is_exported():
    import inspect
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.eval_utils import eval_recommendation
    from www2023tiger_amd.model.tiger import TIGE
    sig = inspect.signature(TIGE.recommend)
    assert list(sig.parameters)[:5] == ['self', 'src_ids', 'ts', 'cand', 'k']
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY
               for n in ('mask', 'exclude_seen', 'graph', 'chunk_queries', 'col_of'))
    assert sig.parameters['chunk_queries'].default == 65536 and sig.parameters['exclude_seen'].default is False
    sig = inspect.signature(eval_recommendation)
    assert list(sig.parameters)[:4] == ['model', 'dl', 'device', 'catalogue']
    assert sig.parameters['k'].default == 10 and sig.parameters['chunk_queries'].default == 65536
    assert hasattr(TIGE, '_pair_scores')
    for name in ('topk_rows', 'catalogue_index', 'seen_mask'):
        assert callable(getattr(hip_ops, name))


def test_catalogue_index():
    from www2023tiger_amd import hip_ops
    cat = torch.tensor([7, 3, 9, 1])
    col_of = hip_ops.catalogue_index(cat, 12)
    assert col_of.dtype == torch.int32 and col_of.tolist() == [-1, 3, -1, 1, -1, -1, -1, 0, -1, 2, -1, -1]
    with pytest.raises(ValueError, match='duplicate'):
        hip_ops.catalogue_index(torch.tensor([7, 3, 7]), 12)
    with pytest.raises(ValueError, match='outside'):
        hip_ops.catalogue_index(torch.tensor([7, 12]), 12)
    with pytest.raises(ValueError, match='outside'):
        hip_ops.catalogue_index(torch.tensor([-1, 2]), 12)
    assert hip_ops.catalogue_index(torch.zeros(0, dtype=torch.int64), 3).tolist() == [-1, -1, -1]


# ---- seen mask ---------------------------------------------------------------------------------------------------------
def host_graph():
    from www2023tiger_amd.data.graph import Graph
    es, ed, et, n = seen_graph()
    return Graph.from_arrays(es, ed, et, np.arange(1, len(es) + 1), strategy='recent_edges', max_node_id=n - 1), (es, ed, et)


def test_seen_mask_host_twin_equals_the_loop():
    from www2023tiger_amd import hip_ops
    g, ev = host_graph()
    deg = np.diff(g._h_indptr)
    assert [int(deg[s]) for s in (1, 2, 3, 4, 5)] == [63, 64, 65, 200, 0]
    src, ts, cat = seen_queries()
    col_of = hip_ops.catalogue_index(t(cat), g.num_node)
    want = numpy_seen_mask(*ev, src, ts, cat)
    got = hip_ops.seen_mask(g, t(src), t(ts), col_of, len(cat))
    assert got.dtype == torch.bool
    np.testing.assert_array_equal(got.numpy(), want)
    assert want[src == 5].all() and want[ts == 0.0].all() and want[ts == 1.0].all()   # nothing before: nothing cleared
    assert (~want).sum() > 50 and not want[(src == 4) & (ts == 101.0)].all()
    # a caller's mask: what it had cleared stays cleared, and it is not written
    mine = np.random.RandomState(1).rand(*want.shape) > 0.3
    keep = mine.copy()
    got = hip_ops.seen_mask(g, t(src), t(ts), col_of, len(cat), mask=t(mine))
    np.testing.assert_array_equal(got.numpy(), numpy_seen_mask(*ev, src, ts, cat, mask=mine))
    np.testing.assert_array_equal(got.numpy(), want & mine)
    np.testing.assert_array_equal(mine, keep)


def test_seen_mask_refuses_bad_arguments():
    from www2023tiger_amd import _lib, hip_ops
    g, _ = host_graph()
    src, ts, cat = seen_queries()
    col_of = hip_ops.catalogue_index(t(cat), g.num_node)
    with pytest.raises(ValueError, match='outside'):
        hip_ops.seen_mask(g, torch.tensor([1, g.num_node]), torch.tensor([1.0, 1.0]), col_of, len(cat))
    with pytest.raises(ValueError, match='col_of'):
        hip_ops.seen_mask(g, t(src), t(ts), col_of[:-1], len(cat))
    h = g._host_tcsr()
    tc = _lib.TgTcsr(g.num_node, len(h[1]), *(_lib.ptr(a) for a in h))
    m = np.ones((2, len(cat)), dtype=np.uint8)
    bad = np.array([1, g.num_node], dtype=np.int64)
    two = np.array([5.0, 5.0])
    p, ref = _lib.ptr, ctypes.byref(tc)
    assert _lib.lib.tg_seen_mask_host(ref, 2, p(bad), p(two), len(cat), p(col_of), p(m)) == _lib.TG_EINVAL
    assert m.all()
    assert _lib.lib.tg_seen_mask_host(ref, -1, p(bad), p(two), len(cat), p(col_of), p(m)) == _lib.TG_EINVAL
    assert _lib.lib.tg_seen_mask_host(None, 2, p(bad), p(two), len(cat), p(col_of), p(m)) == _lib.TG_EINVAL
    assert _lib.lib.tg_seen_mask(None, 2, None, None, 3, None, None, None) == _lib.TG_EINVAL
    assert _lib.lib.tg_seen_mask(ref, 2, None, None, 3, None, None, None) == _lib.TG_EINVAL
    assert _lib.lib.tg_seen_mask(ref, 0, None, None, 3, None, None, None) == _lib.TG_OK
