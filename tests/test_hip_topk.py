"""tg_topk_rows and tg_seen_mask on the GPU against their host twins and the numpy references of tests/_topk_ref.py, bit
for bit: the feature has no tolerance.  Every (B, C) runs k in {1, 10, 63, 64} (k > C and k > n_valid included) and
n_seg in {0, 1, 2, 7, C + 3}, whose results must be identical; scores live in a wider NaN-filled matrix (ld > C), the
outputs are followed by guard words, the workspace starts as NaN bytes."""
import ctypes

import numpy as np
import pytest
import torch

from _topk_ref import (GUARD_F32, GUARD_I32, GUARD_I64, assert_same_topk, numpy_seen_mask, numpy_topk, seen_graph,
                       seen_queries, topk_case)

pytestmark = pytest.mark.gpu
KS = (1, 10, 63, 64)
TAIL = 24   # guard words behind every output


def dev():
    return torch.device('cuda', 0)


def device_topk(s, cand, mask, k, n_seg):
    """the C entry itself: guarded outputs, a NaN-filled workspace of exactly the bytes asked for"""
    from www2023tiger_amd import _lib
    from www2023tiger_amd.hip_ops import stream_ptr
    lib, p = _lib.lib, _lib.ptr
    B, C = s.shape
    guard = lambda n, value, dt: torch.full((n + TAIL,), value, dtype=dt, device=dev())
    ids, sc, cols = guard(B * k, int(GUARD_I64), torch.int64), guard(B * k, float(GUARD_F32), torch.float32), \
        guard(B * k, int(GUARD_I32), torch.int32)
    nv, bad = guard(B, int(GUARD_I32), torch.int32), torch.zeros(1 + TAIL, dtype=torch.int64, device=dev())
    bad[1:] = int(GUARD_I64)
    nbytes = int(lib.tg_topk_rows_workspace_bytes(B, C, k, n_seg))
    ws = torch.full((nbytes + TAIL,), 0xFF, dtype=torch.uint8, device=dev())   # as floats: NaN; as keys: the largest
    ld = s.stride(0) if B > 1 else C
    _lib.check(lib.tg_topk_rows(B, C, k, p(s), ld, p(cand), 1 if cand.dim() == 1 else 0, p(mask), n_seg, p(ids), p(sc),
                                p(cols), p(nv), p(bad), p(ws) if nbytes else None, nbytes, stream_ptr(dev())), 'tg_topk_rows')
    assert (ids[B * k:] == int(GUARD_I64)).all() and (cols[B * k:] == int(GUARD_I32)).all() and (nv[B:] == int(GUARD_I32)).all()
    assert (sc[B * k:] == float(GUARD_F32)).all() and (bad[1:] == int(GUARD_I64)).all() and (ws[nbytes:] == 0xFF).all()
    return dict(ids=ids[:B * k].view(B, k).cpu().numpy(), scores=sc[:B * k].view(B, k).cpu().numpy(),
                cols=cols[:B * k].view(B, k).cpu().numpy(), n_valid=nv[:B].cpu().numpy(), n_nonfinite=bad[:1].cpu().numpy())


VARIANTS = [(True, True), (False, True), (False, False)]   # (shared ids, with a mask)


@pytest.mark.parametrize('C', [1, 63, 64, 65, 129, 1000, 4099])
@pytest.mark.parametrize('B', [1, 3, 65])
def test_device_equals_host_twin_and_numpy_for_every_segment_count(B, C):
    from www2023tiger_amd import hip_ops
    for v, (shared, with_mask) in enumerate(VARIANTS):
        # (a single row takes another kind per variant; 65 rows hold every kind many times)
        s, cand, mask = topk_case(B, C, shared=shared, with_mask=with_mask, ld=C + 3, seed=v, first_kind=v)
        ds, dc = torch.from_numpy(s).to(dev()), torch.from_numpy(cand).to(dev())
        full = torch.full((B, C + 3), float('nan'), device=dev())
        full[:, :C] = ds
        ds = full[:, :C]   # row stride C + 3, NaN behind every row
        dm = None if mask is None else torch.from_numpy(mask).to(dev()).to(torch.uint8)
        for k in KS:
            want = numpy_topk(s, cand, k, mask)
            host = hip_ops.topk_rows(torch.from_numpy(s), torch.from_numpy(cand), k, mask=None if mask is None else torch.from_numpy(mask))
            assert_same_topk({key: val.numpy() for key, val in host.items()}, want, f'host twin k={k}')
            for n_seg in (0, 1, 2, 7, C + 3):
                assert_same_topk(device_topk(ds, dc, dm, k, n_seg), want, f'shared={shared} mask={with_mask} k={k} n_seg={n_seg}')
        if B == 65:
            assert want['n_nonfinite'] > 0 and (want['n_valid'] == 0).sum() >= 20 and want['n_valid'].max() > 0


@pytest.mark.parametrize('B,C,k', [(1, 8200, 64), (2, 8200, 10), (65, 200, 10)])
def test_the_wrapper_with_the_library_chosen_segments(B, C, k):
    """hip_ops.topk_rows (n_seg = 0) where the library splits rows - (1, 8200, 64): 11 segments, (2, 8200, 10): 28 - and
    where it does not; a strided view and the accumulated counter"""
    from www2023tiger_amd import _lib, hip_ops
    chosen = int(_lib.lib.tg_topk_rows_workspace_bytes(B, C, k, 0)) // (B * (8 * k + 8))
    assert (chosen > 1) == (B < 65)
    s, cand, mask = topk_case(B, C, shared=False, with_mask=True, ld=C + 1, first_kind=0)
    want = numpy_topk(s, cand, k, mask)
    acc = torch.zeros(1, dtype=torch.int64, device=dev())
    full = torch.from_numpy(np.ascontiguousarray(s.base if s.base is not None else s)).to(dev())
    got = hip_ops.topk_rows(full[:, :C], torch.from_numpy(cand).to(dev()), k, mask=torch.from_numpy(mask).to(dev()), acc=acc)
    assert got['n_nonfinite'] is acc
    assert_same_topk({key: val.cpu().numpy() for key, val in got.items()}, want)
    hip_ops.topk_rows(full[:, :C], torch.from_numpy(cand).to(dev()), k, mask=torch.from_numpy(mask).to(dev()), acc=acc)
    assert int(acc) == 2 * want['n_nonfinite']


def test_no_columns_and_no_rows():
    from www2023tiger_amd import hip_ops
    out = hip_ops.topk_rows(torch.zeros(3, 0, device=dev()), torch.zeros(0, dtype=torch.int64, device=dev()), 5)
    assert (out['ids'] == 0).all() and torch.isneginf(out['scores']).all() and (out['cols'] == -1).all()
    assert (out['n_valid'] == 0).all() and int(out['n_nonfinite']) == 0
    out = hip_ops.topk_rows(torch.zeros(0, 9, device=dev()), torch.zeros(9, dtype=torch.int64, device=dev()), 5)
    assert out['ids'].shape == (0, 5)


# ---- seen mask ---------------------------------------------------------------------------------------------------------
def test_seen_mask_equals_the_loop_and_the_host_twin():
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.data.graph import Graph
    es, ed, et, n = seen_graph()
    eids = np.arange(1, len(es) + 1)
    g = Graph.from_arrays(es, ed, et, eids, strategy='recent_edges', max_node_id=n - 1, device=dev())
    gh = Graph.from_arrays(es, ed, et, eids, strategy='recent_edges', max_node_id=n - 1)
    src, ts, cat = seen_queries()
    t = lambda a: torch.from_numpy(a).to(dev())
    col_of = hip_ops.catalogue_index(t(cat), n)
    assert col_of.device.type == 'cuda'
    want = numpy_seen_mask(es, ed, et, src, ts, cat)
    got = hip_ops.seen_mask(g, t(src), t(ts), col_of, len(cat))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    host = hip_ops.seen_mask(gh, torch.from_numpy(src), torch.from_numpy(ts), col_of.cpu(), len(cat))
    assert torch.equal(host, got.cpu())
    assert want[src == 5].all() and want[ts == 1.0].all() and (~want).sum() > 50
    mine = np.random.RandomState(1).rand(*want.shape) > 0.3   # the caller's cleared columns stay cleared
    dm = t(mine)
    got = hip_ops.seen_mask(g, t(src), t(ts), col_of, len(cat), mask=dm)
    np.testing.assert_array_equal(got.cpu().numpy(), numpy_seen_mask(es, ed, et, src, ts, cat, mask=mine))
    np.testing.assert_array_equal(dm.cpu().numpy(), mine)
    with pytest.raises(ValueError, match='outside'):
        hip_ops.seen_mask(g, t(np.array([1, n])), t(np.array([1.0, 1.0])), col_of, len(cat))


def test_seen_mask_bytes_behind_the_mask_stay():
    """the C entry on a guarded buffer: only bytes of [B, C] are written, and only cleared"""
    from www2023tiger_amd import _lib, hip_ops
    from www2023tiger_amd.data.graph import Graph
    es, ed, et, n = seen_graph()
    g = Graph.from_arrays(es, ed, et, np.arange(1, len(es) + 1), strategy='recent_edges', max_node_id=n - 1, device=dev())
    src, ts, cat = seen_queries()
    t = lambda a: torch.from_numpy(a).to(dev())
    col_of = hip_ops.catalogue_index(t(cat), n)
    B, C = len(src), len(cat)
    buf = torch.full((B * C + 64,), 7, dtype=torch.uint8, device=dev())
    dsrc, dts = t(src), t(ts)
    p = _lib.ptr
    _lib.check(_lib.lib.tg_seen_mask(ctypes.byref(g.tcsr), B, p(dsrc), p(dts), C, p(col_of), p(buf), hip_ops.stream_ptr(dev())),
               'tg_seen_mask')
    got = buf.cpu().numpy()
    assert (got[B * C:] == 7).all() and set(np.unique(got[:B * C]).tolist()) == {0, 7}
    np.testing.assert_array_equal(got[:B * C].reshape(B, C) == 7, numpy_seen_mask(es, ed, et, src, ts, cat))
