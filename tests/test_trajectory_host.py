"""Trajectory encoding without a GPU: the host twins of tg_trajectory_accumulate / tg_trajectory_finish against the
reference's own tables (tests/golden/trajectory_*.npz, written by make_trajectory_golden.py from the reference's
encode_trajectory) and against a plain sequential float64 loop on random inputs with dense id collisions."""
import ctypes

import numpy as np
import pytest

from _util import load, parse_cfg

FIXTURES = ['trajectory_seq_lr_d8', 'trajectory_static_ll_d16']
CASES = [('last', True, True), ('max', True, True), ('mean', True, True), ('sum', True, True), ('mean', False, True),
         ('mean', True, False)]
RANDOM_D = [4, 8, 100, 172, 256]
RANDOM_B = [1, 50, 200, 1024, 5000]


def mode_of(agg):
    from www2023tiger_amd import _lib
    return {'last': _lib.TG_TRAJ_LAST, 'max': _lib.TG_TRAJ_MAX}.get(agg, _lib.TG_TRAJ_SUM)


def host_accumulate(h, src, dst, mode, use_src, use_dst, table, counts, err, offset=None):
    from www2023tiger_amd._lib import lib, ptr
    B = len(h) // 2
    assert h.dtype == np.float32 and h.flags.c_contiguous and src.dtype == np.int64 and dst.dtype == np.int64
    assert table.dtype == np.float64 and counts.dtype == np.float64 and err.dtype == np.uint32
    off = None if offset is None else np.array([offset], dtype=np.int64)
    rc = lib.tg_trajectory_accumulate_host(B, h.shape[1], ptr(h), ptr(src), ptr(dst), ptr(off), mode, int(use_src),
                                           int(use_dst), len(table), ptr(table), ptr(counts), ptr(err))
    assert rc == 0


def host_finish(table, counts):
    from www2023tiger_amd._lib import lib, ptr
    assert lib.tg_trajectory_finish_host(len(table), table.shape[1], ptr(table), ptr(counts)) == 0


def loop_accumulate(h, src, dst, agg, use_src, use_dst, table, counts):
    """the sequential float64 loop: sources in index order, then destinations; a bad id is skipped"""
    B, n = len(h) // 2, len(table)
    if use_src:
        for i, node in enumerate(src[:B]):
            if not 0 <= node < n:
                continue
            if agg == 'last':
                table[node] = h[i]
            elif agg == 'max':
                table[node] = np.maximum(table[node], h[i])
            else:
                table[node] += h[i]
            counts[node] += 1
    if use_dst:
        for j, node in enumerate(dst[:B]):
            if not 0 <= node < n:
                continue
            if agg == 'max':
                table[node] = np.maximum(table[node], h[B + j])
            else:
                table[node] = h[B + j]
            counts[node] += 1


def random_case(d, B, seed, n_batches=3):
    """ids from a small range (dense collisions, nodes on both sides of a batch), a few batches over one table"""
    rs = np.random.RandomState(seed)
    n_nodes = max(2, min(97, B // 3 + 2))
    batches = []
    for _ in range(n_batches):
        h = rs.standard_normal((2 * B, d)).astype(np.float32)
        batches.append((h, rs.randint(0, n_nodes, B).astype(np.int64), rs.randint(0, n_nodes, B).astype(np.int64)))
    return n_nodes, batches


def fresh(n_nodes, d):
    return np.zeros((n_nodes, d)), np.zeros(n_nodes), np.zeros(1, dtype=np.uint32)


@pytest.mark.parametrize('name', FIXTURES)
def test_host_twin_reproduces_the_reference_tables_bit_for_bit(name):
    """the recorded h and ids of every batch through the host twin and its finish: the reference's table for every
    recorded (agg, use_src, use_dst) - order within a batch, `=` against `+=`, the division of 'mean' alone"""
    z = load(name)
    cfg = parse_cfg(z)
    B, d, n_nodes = cfg['B'], cfg['d'], int(z['n_nodes'])
    src, dst = z['src'], z['dst']
    hs = [z[f'b{b}_h'] for b in range(int(z['n_batches']))]
    assert sum(len(h) for h in hs) == 2 * len(src)
    for agg, use_src, use_dst in CASES:
        table, counts, err = fresh(n_nodes, d)
        for b, h in enumerate(hs):
            s = np.ascontiguousarray(src[b * B:(b + 1) * B])
            t = np.ascontiguousarray(dst[b * B:(b + 1) * B])
            assert len(h) == 2 * len(s)
            host_accumulate(h, s, t, mode_of(agg), use_src, use_dst, table, counts, err)
        assert int(err[0]) == 0
        if agg == 'mean':
            host_finish(table, counts)
        want = z[f'table_{agg}_src{int(use_src)}_dst{int(use_dst)}']
        assert want.dtype == np.float64 and want.shape == (n_nodes, d)
        assert np.array_equal(table, want), (agg, use_src, use_dst)
    # the fixture distinguishes the modes: 'sum' is not 'last' (a source row was added), 'max' clipped at zero
    assert not np.array_equal(z['table_sum_src1_dst1'], z['table_last_src1_dst1'])
    assert (z['table_last_src1_dst1'] < 0).any() and (z['table_max_src1_dst1'] >= 0).all()


@pytest.mark.parametrize('d', RANDOM_D)
@pytest.mark.parametrize('B', RANDOM_B)
def test_host_twin_equals_a_sequential_float64_loop(d, B):
    n_nodes, batches = random_case(d, B, seed=1000 * d + B)
    for agg, use_src, use_dst in CASES + [('last', False, True), ('max', True, False)]:
        table, counts, err = fresh(n_nodes, d)
        want, want_counts = np.zeros((n_nodes, d)), np.zeros(n_nodes)
        for h, s, t in batches:
            host_accumulate(h, s, t, mode_of(agg), use_src, use_dst, table, counts, err)
            loop_accumulate(h, s, t, agg, use_src, use_dst, want, want_counts)
        assert int(err[0]) == 0
        assert np.array_equal(counts, want_counts)
        if agg == 'mean':
            host_finish(table, counts)
            want /= want_counts[:, None] + 1e-7
        assert np.array_equal(table, want), (agg, use_src, use_dst)


def test_ids_are_read_at_the_offset():
    """id columns of a whole stream with the batch at an element offset (the resident form)"""
    d, B = 8, 50
    n_nodes, batches = random_case(d, B, seed=7)
    src = np.concatenate([s for _, s, _ in batches])
    dst = np.concatenate([t for _, _, t in batches])
    table, counts, err = fresh(n_nodes, d)
    want, want_counts = np.zeros((n_nodes, d)), np.zeros(n_nodes)
    for b, (h, s, t) in enumerate(batches):
        host_accumulate(h, src, dst, mode_of('sum'), True, True, table, counts, err, offset=b * B)
        loop_accumulate(h, s, t, 'sum', True, True, want, want_counts)
    assert np.array_equal(table, want) and np.array_equal(counts, want_counts)


def test_out_of_range_ids_set_the_error_word_and_are_skipped():
    from www2023tiger_amd import _lib
    d, B = 8, 200
    n_nodes, ((h, s, t),) = random_case(d, B, seed=3, n_batches=1)
    s, t = s.copy(), t.copy()
    s[[3, 77]] = [-1, n_nodes]
    t[[0, 150]] = [n_nodes + 5, -(2 ** 40)]
    for agg in ('last', 'max', 'mean'):
        # guard rows on both sides of the table: an out-of-range store would land there
        buf = np.full((n_nodes + 16, d), 7.0)
        buf[8:8 + n_nodes] = 0
        table = buf[8:8 + n_nodes]
        cbuf = np.full(n_nodes + 16, 7.0)
        cbuf[8:8 + n_nodes] = 0
        counts = cbuf[8:8 + n_nodes]
        err = np.zeros(1, dtype=np.uint32)
        host_accumulate(h, s, t, mode_of(agg), True, True, table, counts, err)
        assert int(err[0]) == _lib.TG_TRAJ_ERR_BAD_ID
        want, want_counts = np.zeros((n_nodes, d)), np.zeros(n_nodes)
        loop_accumulate(h, s, t, agg, True, True, want, want_counts)
        assert np.array_equal(table, want) and np.array_equal(counts, want_counts)
        assert (buf[:8] == 7).all() and (buf[8 + n_nodes:] == 7).all()
        assert (cbuf[:8] == 7).all() and (cbuf[8 + n_nodes:] == 7).all()
        assert counts.sum() == 2 * B - 4


def test_entry_points_refuse_bad_arguments():
    from www2023tiger_amd import _lib
    lib = _lib.lib
    one = np.zeros(8)
    e = np.zeros(1, dtype=np.uint32)
    p = _lib.ptr
    for B, d, mode, n in ((-1, 4, 0, 2), (1, 0, 0, 2), (1, 4, 3, 2), (1, 4, -1, 2), (1, 4, 0, 0)):
        assert lib.tg_trajectory_accumulate_host(B, d, p(one), p(one), p(one), None, mode, 1, 1, n, p(one), p(one), p(e)) == _lib.TG_EINVAL
        assert lib.tg_trajectory_accumulate(B, d, None, None, None, None, mode, 1, 1, n, None, None, None, None) == _lib.TG_EINVAL
    assert lib.tg_trajectory_accumulate(4, 4, None, None, None, None, 0, 1, 1, 2, None, None, None, None) == _lib.TG_EINVAL
    assert lib.tg_trajectory_accumulate(0, 4, None, None, None, None, 0, 1, 1, 2, None, None, None, None) == _lib.TG_OK
    assert lib.tg_trajectory_accumulate(4, 4, None, None, None, None, 0, 0, 0, 2, None, None, None, None) == _lib.TG_OK
    assert lib.tg_trajectory_finish_host(2, 0, p(one), p(one)) == _lib.TG_EINVAL
    assert lib.tg_trajectory_finish(2, 4, None, None, None) == _lib.TG_EINVAL


def test_symbols_resolve_and_the_abi_version_stays():
    from www2023tiger_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('tg_trajectory_accumulate', 'tg_trajectory_finish', 'tg_trajectory_accumulate_host',
                 'tg_trajectory_finish_host'):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.lib.tg_abi_version() == 9


def test_encode_trajectory_is_exported_with_the_reference_signature():
    import inspect
    from www2023tiger_amd.eval_utils import encode_trajectory
    sig = inspect.signature(encode_trajectory)
    assert list(sig.parameters) == ['model', 'dl', 'device', 'agg', 'use_src', 'use_dst', 'as_tensor']
    assert sig.parameters['use_src'].default is True and sig.parameters['use_dst'].default is True
    assert sig.parameters['as_tensor'].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters['as_tensor'].default is False
