"""Embedding nearest neighbours on the GPU: tg_knn_rows (selection on the MFMA accumulators) against int64 numpy on the
exact family and against the host twin, bit for bit, on the float family - at the tile, wavefront, width and split edges
of tests/_knn_ref.py, with guards past the outputs.  The refusals of the device entry and its workspace."""
import numpy as np
import pytest
import torch

from _knn_ref import (CT, QT, SHAPE_IDS, SHAPES, case_tensors, exact_scores, knn_case, reference_topk, run_knn, twin_topk)
from _topk_ref import assert_same_topk
from test_knn_host import REFUSALS, assert_refused, flat
from www2023tiger_amd import _lib, hip_ops
from www2023tiger_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_SPLITS = (0, 1, 2, 3, 1000)   # 1000: more splits than any case here has catalogue tiles


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_exact_family_equals_int64_numpy(shape):
    Q, C, d, k, ns, opts = shape
    case = knn_case(Q, C, d, 'exact', opts)
    want = reference_topk(case, exact_scores(case), k)
    for n_split in sorted({ns, 0, 3}):
        rc, res = run_knn(case, k, n_split, DEV)
        assert rc == _lib.TG_OK
        assert_same_topk(flat(res), want, f'{shape} n_split={n_split}')


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_float_family_equals_the_twin(shape):
    Q, C, d, k, ns, opts = shape
    case = knn_case(Q, C, d, 'float', opts)
    want = twin_topk(Q, C, d, k, 'float', opts)
    for n_split in sorted({ns, 0, 2}):
        rc, res = run_knn(case, k, n_split, DEV)
        assert rc == _lib.TG_OK
        assert_same_topk(flat(res), want, f'{shape} n_split={n_split}')


@pytest.mark.parametrize('family', ['exact', 'float'])
@pytest.mark.parametrize('k', [1, 10, 64])
def test_every_n_split_and_k_give_the_same_bits(family, k):
    """two query tiles and a half against nine catalogue tiles and one column; every split count, empty splits included"""
    Q, C, d = 2 * QT + 1, 9 * CT + 1, 36
    case = knn_case(Q, C, d, family, '')
    want = twin_topk(Q, C, d, k, family, '')
    for n_split in N_SPLITS:
        rc, res = run_knn(case, k, n_split, DEV)
        assert rc == _lib.TG_OK
        assert_same_topk(flat(res), want, f'n_split={n_split}')


@pytest.mark.parametrize('kind', ['dup', 'mask_zero', 'k_above_C'])
def test_exact_family_constructed(kind):
    Q, C, d, k = (9, 5, 8, 64) if kind == 'k_above_C' else (9, 70, 8, 10)
    case = knn_case(Q, C, d, 'exact', '', mask='zero' if kind == 'mask_zero' else 'random', dup=kind == 'dup')
    want = reference_topk(case, exact_scores(case), k)
    for n_split in (0, 2):
        rc, res = run_knn(case, k, n_split, DEV)
        assert rc == _lib.TG_OK
        assert_same_topk(flat(res), want, kind)


def test_increasing_scores_insert_every_column():
    """q = e0 against c[j, 0] = j over 65 tiles: every tile beats every threshold, for k = 64 and both tile heights"""
    for d in (8, 288):
        case = knn_case(10, 4097, d, 'exact', 'plain')
        want = reference_topk(case, exact_scores(case), 64)
        np.testing.assert_array_equal(want['cols'][1], np.arange(4096, 4032, -1))
        rc, res = run_knn(case, 64, 1, DEV)
        assert rc == _lib.TG_OK
        assert_same_topk(flat(res), want, f'd={d}')


def test_wrapper_on_the_device_and_the_accumulator():
    case = knn_case(33, 2 * CT + 1, 172, 'float', 'pad')
    want = twin_topk(33, 2 * CT + 1, 172, 10, 'float', 'pad')
    t = case_tensors(case, DEV)
    t['col_mask'] = t['col_mask'].bool()
    acc = torch.full((1,), 1000, dtype=torch.int64, device=DEV)
    out = hip_ops.knn_rows(t.pop('q'), t.pop('c'), 10, acc=acc, **t)
    got = {key: v.cpu().numpy() for key, v in out.items()}
    got['n_nonfinite'] = got['n_nonfinite'] - 1000
    assert_same_topk(got, want)
    with pytest.raises(ValueError):
        hip_ops.knn_rows(torch.zeros(3, 8, device=DEV), torch.zeros(5, 8), 4)   # tensors on different devices


@pytest.mark.parametrize('change,code', REFUSALS, ids=[str(sorted(c.items())) for c, _ in REFUSALS])
def test_device_refusals_write_nothing(change, code):
    assert_refused(change, code, DEV)


def test_short_workspace_and_empty_shapes():
    case = knn_case(33, 33, 172, 'exact', '')
    for n_split in (0, 1, 3):
        rc, res = run_knn(case, 10, n_split, DEV, ws_short=1)
        assert rc == _lib.TG_EWORKSPACE
        assert (res['ids_all'] < 0).all() and (res['cols_all'] < -1).all()   # the guards: nothing was written
    assert int(lib.tg_knn_rows_workspace_bytes(33, 33, 10, 3)) == 33 * 3 * (10 * 8 + 8)
    rc, res = run_knn(knn_case(0, 33, 4, 'exact'), 3, 0, DEV)
    assert rc == _lib.TG_OK and (res['ids_all'] < 0).all()
    rc, res = run_knn(knn_case(4, 0, 8, 'exact'), 3, 2, DEV)
    assert rc == _lib.TG_OK and (res['ids'] == 0).all() and (res['cols'] == -1).all() \
        and np.isneginf(res['scores']).all() and (res['n_valid'] == 0).all()
