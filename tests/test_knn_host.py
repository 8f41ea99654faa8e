"""Embedding nearest neighbours without a GPU: the host twin tg_knn_rows_host against numpy (tests/_knn_ref.py) - the exact
family against int64 arithmetic plus numpy_topk, bit for bit; the float family's full matrix against float64 within the
fma-chain bound and its lists against numpy_topk on the twin's own bits.  The ABI: symbols, version, every refusal of
either entry before anything is written, the workspace size."""
import numpy as np
import pytest
import torch

from _knn_ref import (CT, QT, SHAPE_IDS, SHAPES, exact_scores, float64_scores, knn_case, reference_topk, run_knn,
                      untouched)
from _topk_ref import assert_same_topk
from www2023tiger_amd import _lib, hip_ops
from www2023tiger_amd._lib import lib


def flat(res):
    return {key: res[key] for key in ('ids', 'scores', 'cols', 'n_valid', 'n_nonfinite')}


def test_symbols_and_version():
    for name in ('tg_knn_rows', 'tg_knn_rows_host', 'tg_knn_rows_workspace_bytes'):
        assert getattr(lib, name)
    assert lib.tg_abi_version() == 9
    assert (QT, CT) == (128, 64) and _lib.TG_TOPK_MAX_K == 64


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_exact_family_equals_int64_numpy(shape):
    Q, C, d, k, ns, opts = shape
    case = knn_case(Q, C, d, 'exact', opts)
    rc, res, matrix = run_knn(case, k, ns, want_matrix=True)
    assert rc == _lib.TG_OK
    want_s = exact_scores(case)
    np.testing.assert_array_equal(matrix.view(np.uint32), want_s.view(np.uint32))
    assert_same_topk(flat(res), reference_topk(case, want_s, k), f'{shape}')


@pytest.mark.parametrize('kind', ['dup', 'mask_zero', 'k_above_C'])
def test_exact_family_constructed(kind):
    """duplicate catalogue rows (ties by ascending column), a col_mask of zeros (every position is padding), k > C"""
    Q, C, d, k = (9, 5, 8, 64) if kind == 'k_above_C' else (9, 70, 8, 10)
    case = knn_case(Q, C, d, 'exact', '', mask='zero' if kind == 'mask_zero' else 'random', dup=kind == 'dup')
    rc, res = run_knn(case, k, 0)
    assert rc == _lib.TG_OK
    want = reference_topk(case, exact_scores(case), k)
    assert_same_topk(flat(res), want, kind)
    if kind == 'mask_zero':
        assert (res['n_valid'] == 0).all() and (res['ids'] == 0).all() and (res['cols'] == -1).all() \
            and np.isneginf(res['scores']).all()
    if kind == 'k_above_C':
        assert (res['cols'][:, C:] == -1).all()
    if kind == 'dup':   # the three equal rows 3, 5, 6 come in column order wherever all three are listed
        for i in range(Q):
            pos = [int(np.nonzero(res['cols'][i] == j)[0][0]) for j in (3, 5, 6) if (res['cols'][i] == j).any()]
            assert pos == sorted(pos)


def test_exact_family_order_of_constructed_rows():
    """q = e0: strictly increasing scores -> the LAST columns, descending; q = -e0: the first, ascending; q = e1: all equal
    -> the first columns left in, ascending"""
    case = knn_case(10, 4 * CT + 1, 8, 'exact', 'plain')
    rc, res = run_knn(case, 10, 0)
    assert rc == _lib.TG_OK
    C = case['C']
    np.testing.assert_array_equal(res['cols'][1], np.arange(C - 1, C - 11, -1))
    np.testing.assert_array_equal(res['cols'][2], np.arange(10))
    np.testing.assert_array_equal(res['cols'][3], np.arange(10))
    np.testing.assert_array_equal(res['ids'][3], np.arange(1, 11))   # ids NULL: column + 1


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_float_family_matrix_and_lists(shape):
    Q, C, d, k, ns, opts = shape
    case = knn_case(Q, C, d, 'float', opts)
    rc, res, S = run_knn(case, k, ns, want_matrix=True)
    assert rc == _lib.TG_OK
    S64, bound, finite = float64_scores(case)
    err = np.abs(S.astype(np.float64) - S64)
    worst = float((err[finite] / np.maximum(bound[finite], 1e-300)).max(initial=0.0))
    print(f'{shape}: worst |S - S64| / bound = {worst:.3f}, {int((~finite).sum())} pairs with a non-finite operand')
    assert np.isfinite(S[finite]).all() and (err[finite] <= bound[finite]).all()
    # a NaN / inf operand entry leaves no finite score (inf x 0 is NaN, and neither scale brings it back)
    assert not np.isfinite(S[~finite]).any()
    assert_same_topk(flat(res), reference_topk(case, S, k), f'{shape}')
    if Q * C >= 8000:   # the case says what it was made to say
        assert int(res['n_nonfinite'][0]) > 0 and (~finite).any() and finite.any()


def test_n_split_does_not_matter_on_the_host_and_accumulates():
    case = knn_case(5, 200, 8, 'float', '')
    _, a = run_knn(case, 10, 0)
    _, b = run_knn(case, 10, 9)
    assert_same_topk(flat(a), {**flat(b), 'n_nonfinite': int(b['n_nonfinite'][0])})
    t = {key: None if v is None else torch.tensor(np.ascontiguousarray(v)) for key, v in case.items()
         if key in ('q', 'c', 'ids', 'q_scale', 'c_scale', 'exclude', 'col_mask')}
    q, c = t.pop('q'), t.pop('c')
    acc = torch.full((1,), 1000, dtype=torch.int64)
    out = hip_ops.knn_rows(q, c, 10, acc=acc, **t)
    assert out['n_nonfinite'] is acc and int(acc) == 1000 + int(a['n_nonfinite'][0])
    for key in ('ids', 'cols', 'n_valid'):
        np.testing.assert_array_equal(out[key].numpy(), a[key])


REFUSALS = [   # (what to change, the code)
    (dict(Q=-1), _lib.TG_EINVAL), (dict(C=-1), _lib.TG_EINVAL), (dict(C=1 << 31), _lib.TG_EINVAL),
    (dict(d=-4), _lib.TG_EINVAL), (dict(ldq=7), _lib.TG_EINVAL), (dict(ldc=7), _lib.TG_EINVAL),
    (dict(k=0), _lib.TG_EINVAL), (dict(k=65), _lib.TG_EINVAL), (dict(n_split=-1), _lib.TG_EINVAL),
    (dict(q=None), _lib.TG_EINVAL), (dict(c=None), _lib.TG_EINVAL), (dict(out_ids=None), _lib.TG_EINVAL),
    (dict(out_scores=None), _lib.TG_EINVAL), (dict(out_cols=None), _lib.TG_EINVAL), (dict(n_valid=None), _lib.TG_EINVAL),
    (dict(n_nonfinite=None), _lib.TG_EINVAL),
    (dict(d=6, ldq=8, ldc=8), _lib.TG_EUNSUPPORTED), (dict(d=516, ldq=516, ldc=516), _lib.TG_EUNSUPPORTED),
    (dict(d=0), _lib.TG_EUNSUPPORTED),
]


def refusal_call(change, device):
    """One call of either entry with `change` applied to a valid argument list (Q 3, C 5, d 8, k 4); the operands are big
    enough for every width asked for, and nothing may be written.  -> (rc, outputs)"""
    from www2023tiger_amd.hip_ops import stream_ptr
    a = dict(Q=3, C=5, d=8, k=4, ldq=8, ldc=8, n_split=0)
    q = torch.ones(3 * 520, device=device)
    c = torch.ones(5 * 520, device=device)
    outs = dict(out_ids=torch.full((3, 4), -7, dtype=torch.int64, device=device),
                out_scores=torch.full((3, 4), -7.0, device=device),
                out_cols=torch.full((3, 4), -7, dtype=torch.int32, device=device),
                n_valid=torch.full((3,), -7, dtype=torch.int32, device=device),
                n_nonfinite=torch.zeros(1, dtype=torch.int64, device=device))
    ptrs = dict(q=q.data_ptr(), c=c.data_ptr(), **{key: v.data_ptr() for key, v in outs.items()})
    a.update(ptrs)
    a.update(change)
    args = (a['Q'], a['C'], a['d'], a['k'], a['q'], a['ldq'], a['c'], a['ldc'], None, None, None, None, None, a['n_split'],
            a['out_ids'], a['out_scores'], a['out_cols'], a['n_valid'], a['n_nonfinite'])
    if device == 'cpu':
        rc = lib.tg_knn_rows_host(*args, None)
    else:
        ws = torch.empty(1 << 16, dtype=torch.uint8, device=device)
        rc = lib.tg_knn_rows(*args, ws.data_ptr(), ws.numel(), stream_ptr(torch.device(device)))
        torch.cuda.synchronize()
    return rc, {key: v.cpu() for key, v in outs.items()}


def assert_refused(change, code, device):
    rc, outs = refusal_call(change, device)
    assert rc == code, (change, rc)
    for key, v in outs.items():
        assert (v == (0 if key == 'n_nonfinite' else -7)).all(), (change, key)


@pytest.mark.parametrize('change,code', REFUSALS, ids=[str(sorted(c.items())) for c, _ in REFUSALS])
def test_host_refusals_write_nothing(change, code):
    assert_refused(change, code, 'cpu')


def test_empty_shapes_on_the_host():
    rc, res = run_knn(knn_case(0, 33, 4, 'exact'), 3, 0)
    assert rc == _lib.TG_OK and untouched(res)            # Q == 0: nothing is written
    rc, res = run_knn(knn_case(4, 0, 8, 'exact'), 3, 2)
    assert rc == _lib.TG_OK and (res['ids'] == 0).all() and (res['cols'] == -1).all() \
        and np.isneginf(res['scores']).all() and (res['n_valid'] == 0).all()


def test_workspace_has_no_term_in_Q_times_C():
    """keys and counts per (row, split): at most 16 bytes per key position, whatever C is"""
    for Q in (1, 64, 1024, 100000):
        for k in (1, 10, 64):
            for ns in (1, 2, 7, 300):
                sizes = {int(lib.tg_knn_rows_workspace_bytes(Q, C, k, ns)) for C in (1, 65536, 1 << 20, (1 << 31) - 1)}
                assert len(sizes) == 1 and 0 < sizes.pop() <= 16 * Q * ns * k
            # the library's own choice: never more than 512 splits a row
            for C in (1, 65536, 1 << 20, (1 << 31) - 1):
                assert 0 < int(lib.tg_knn_rows_workspace_bytes(Q, C, k, 0)) <= 16 * Q * 512 * k
    assert int(lib.tg_knn_rows_workspace_bytes(4, 4, 65, 0)) == 0      # refused arguments size nothing
    assert int(lib.tg_knn_rows_workspace_bytes(4, 4, 4, -1)) == 0


def test_wrapper_refuses_with_value_errors():
    q, c = torch.zeros(3, 8), torch.zeros(5, 8)
    for bad in (lambda: hip_ops.knn_rows(q, c, 0), lambda: hip_ops.knn_rows(q, c, 65),
                lambda: hip_ops.knn_rows(q, c, 4, n_split=-1), lambda: hip_ops.knn_rows(q, torch.zeros(5, 12), 4),
                lambda: hip_ops.knn_rows(torch.zeros(3, 6), torch.zeros(5, 6), 4),
                lambda: hip_ops.knn_rows(torch.zeros(3, 516), torch.zeros(5, 516), 4),
                lambda: hip_ops.knn_rows(q.double(), c, 4), lambda: hip_ops.knn_rows(q, c, 4, ids=torch.zeros(4, dtype=torch.int64)),
                lambda: hip_ops.knn_rows(q, c, 4, exclude=torch.zeros(3, dtype=torch.int32)),
                lambda: hip_ops.knn_rows(q, c, 4, col_mask=torch.ones(6, dtype=torch.bool))):
        with pytest.raises(ValueError):
            bad()
    out = hip_ops.knn_rows(q, c, 4)   # all scores +0.0: columns in order, ids column + 1
    assert out['ids'].tolist() == [[1, 2, 3, 4]] * 3 and out['n_valid'].tolist() == [5, 5, 5]
