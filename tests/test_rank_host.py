"""Rank statistics without a GPU: tg_rank_stats_host (the host twin of tg_rank_stats, same arithmetic) against a numpy
float64 restatement of the definition on a hand-made score matrix - ties with the positive, ties among negatives, an
event with every candidate left out, the three ways a candidate is left out, a cut-off above the candidate count."""
import ctypes

import numpy as np
import pytest
import torch

KS = (1, 3, 10)
B, C = 6, 9


def case():
    """scores [6, 1 + 9], candidate ids, destinations, caller mask"""
    dst = np.array([11, 12, 13, 14, 15, 16], dtype=np.int64)
    cand = np.arange(100, 100 + B * C, dtype=np.int64).reshape(B, C)
    s = np.zeros((B, 1 + C), dtype=np.float32)
    # event 0: a clear rank (2 above, none equal)
    s[0] = [0.5, 0.9, 0.7, 0.1, 0.2, 0.3, -0.4, 0.0, 0.25, 0.45]
    # event 1: exact ties with the positive (3 equal, 1 above)
    s[1] = [0.25, 0.25, 0.25, 0.5, 0.25, 0.0, -1.0, 0.1, 0.2, 0.24999999]
    # event 2: ties among the negatives only (two equal pairs above and below)
    s[2] = [0.0, 1.5, 1.5, -2.0, -2.0, 3.0, 3.0, -0.5, 0.5, -0.25]
    # event 3: every candidate left out - dst itself, the pad id, the caller's mask - though all score above
    s[3] = [-5.0] + [1.0] * C
    cand[3, :3] = dst[3]
    cand[3, 3:6] = 0
    # event 4: leaving out changes the rank: the three best candidates are dst / pad / masked, a tie is masked too
    s[4] = [1.0, 9.0, 8.0, 7.0, 1.0, 1.0, 2.0, 0.5, 0.5, -3.0]
    cand[4, 0] = dst[4]
    cand[4, 1] = 0
    # event 5: the positive is the best; ten candidates do not exist (k = 10 > C)
    s[5] = [4.0, 3.0, 2.0, 1.0, 0.0, -1.0, -2.0, -3.0, -4.0, 3.9999998]
    mask = np.ones((B, C), dtype=bool)
    mask[3, 6:] = False
    mask[4, 2] = False
    mask[4, 3] = False
    return s, cand, dst, mask


def numpy_stats(s, cand, dst, mask, ks=KS):
    """the definition, float64: rank = 1 + #greater + #equal / 2 over the candidates left in"""
    s0 = s[:, :1]
    left_in = (cand != dst[:, None]) & (cand != 0)
    if mask is not None:
        left_in &= mask
    g = ((s[:, 1:] > s0) & left_in).sum(1)
    e = ((s[:, 1:] == s0) & left_in).sum(1)
    rank = 1.0 + g.astype(np.float64) + 0.5 * e.astype(np.float64)
    return dict(n_greater=g, n_equal=e, n_valid=left_in.sum(1), rank=rank, mrr=float(np.mean(1.0 / rank)),
                hits={k: float(np.mean(rank <= k)) for k in ks})


def host_stats(s, cand, dst, mask, ks=KS, acc=None):
    from www2023tiger_amd import hip_ops
    t = torch.from_numpy
    ids = np.concatenate([dst[:, None], cand], 1)
    return hip_ops.rank_stats(t(s), t(ids), t(dst), mask=None if mask is None else t(mask), ks=ks, acc=acc)


@pytest.mark.parametrize('with_mask', [True, False])
def test_host_twin_equals_the_numpy_definition(with_mask):
    from www2023tiger_amd import hip_ops
    s, cand, dst, mask = case()
    mask = mask if with_mask else None
    want = numpy_stats(s, cand, dst, mask)
    got = host_stats(s, cand, dst, mask)
    for k in ('n_greater', 'n_equal', 'n_valid'):
        assert got[k].dtype == torch.int32
        np.testing.assert_array_equal(got[k].numpy(), want[k])
    assert got['rank'].dtype == torch.float64
    np.testing.assert_array_equal(got['rank'].numpy(), want['rank'])
    m = hip_ops.rank_metrics(got['acc'], KS)
    assert m['n_events'] == B
    assert abs(m['mrr'] - want['mrr']) < 1e-12
    for k in KS:
        assert abs(m['hits'][k] - want['hits'][k]) < 1e-12
    assert m['hits'][10] == 1.0  # nobody ranks below 10 among 9 candidates
    if with_mask:  # the hand-made rows say what they were made to say
        assert want['rank'].tolist() == [3.0, 3.5, 6.0, 1.0, 2.5, 1.0]
        assert want['n_valid'].tolist() == [9, 9, 9, 0, 5, 9]
        assert want['n_equal'][1] == 3 and want['n_equal'][2] == 0


def test_the_accumulator_folds_over_calls():
    from www2023tiger_amd import hip_ops
    s, cand, dst, mask = case()
    want = numpy_stats(s, cand, dst, mask)
    acc = hip_ops.new_rank_acc(torch.device('cpu'))
    a = host_stats(s[:4], cand[:4], dst[:4], mask[:4], acc=acc)
    b = host_stats(s[4:], cand[4:], dst[4:], mask[4:], acc=acc)
    assert a['acc'] is acc and b['acc'] is acc
    np.testing.assert_array_equal(np.concatenate([a['rank'].numpy(), b['rank'].numpy()]), want['rank'])
    m = hip_ops.rank_metrics(acc, KS)
    assert m['n_events'] == B and abs(m['mrr'] - want['mrr']) < 1e-12
    assert all(abs(m['hits'][k] - want['hits'][k]) < 1e-12 for k in KS)


def test_a_non_finite_score_is_counted_and_raises():
    from www2023tiger_amd import hip_ops
    s, cand, dst, mask = case()
    s[0, 2] = np.nan       # a candidate left in
    s[5, 0] = np.inf       # a positive
    s[3, 1] = np.nan       # a candidate left out: not ranked, not counted
    got = host_stats(s, cand, dst, mask)
    assert int(got['acc'][1][1]) == 2 and int(got['acc'][1][0]) == B
    with pytest.raises(ValueError, match='2 non-finite'):
        hip_ops.rank_metrics(got['acc'], KS)


def test_entry_points_refuse_bad_arguments():
    from www2023tiger_amd import _lib
    lib, p = _lib.lib, _lib.ptr
    one = np.zeros(16)
    ks = np.array([1, 3, 10], dtype=np.int32)
    a = [p(one)] * 4
    o = [p(one)] * 6
    assert lib.tg_rank_stats_host(-1, 3, *a, 3, p(ks), *o) == _lib.TG_EINVAL
    assert lib.tg_rank_stats_host(2, -1, *a, 3, p(ks), *o) == _lib.TG_EINVAL
    assert lib.tg_rank_stats_host(2, 3, *a, 9, p(ks), *o) == _lib.TG_EINVAL       # more than TG_RANK_MAX_K cut-offs
    assert lib.tg_rank_stats_host(2, 3, *a, 1, p(np.zeros(1, dtype=np.int32)), *o) == _lib.TG_EINVAL  # k < 1
    assert lib.tg_rank_stats_host(2, 3, None, None, None, None, 3, p(ks), *o) == _lib.TG_EINVAL
    assert lib.tg_rank_stats_host(0, 3, None, None, None, None, 3, p(ks), *([None] * 6)) == _lib.TG_OK
    assert lib.tg_rank_stats(2, 3, None, None, None, None, 3, p(ks), *([None] * 6), None) == _lib.TG_EINVAL
    assert lib.tg_rank_stats(2 ** 31, 3, None, None, None, None, 3, p(ks), *([None] * 6), None) == _lib.TG_EINVAL
    sp = _lib.TgScoreParams()
    assert lib.tg_rank_scores(4, 3, 8, 5, ctypes.byref(sp), *([None] * 8), 0, None) == _lib.TG_EINVAL  # no fc1 / fc2
    assert lib.tg_rank_scores_workspace_bytes(4, 8, None) == 0


def test_symbols_resolve_and_the_abi_version_stays():
    from www2023tiger_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('tg_rank_scores', 'tg_rank_scores_workspace_bytes', 'tg_rank_stats', 'tg_rank_stats_host'):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.lib.tg_abi_version() == 9


def test_python_surface_is_exported():
    import inspect
    from www2023tiger_amd.eval_utils import eval_edge_ranking
    from www2023tiger_amd.model.tiger import TIGE
    sig = inspect.signature(eval_edge_ranking)
    assert list(sig.parameters)[:4] == ['model', 'dl', 'device', 'candidates']
    assert sig.parameters['ks'].default == (1, 3, 10) and sig.parameters['restart_mode'].default is False
    assert sig.parameters['chunk_queries'].default == 65536 and sig.parameters['return_ranks'].default is False
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
               for k in ('ks', 'restart_mode', 'mask', 'chunk_queries', 'return_ranks'))
    sig = inspect.signature(TIGE.rank_scores)
    assert list(sig.parameters)[:5] == ['self', 'src_ids', 'dst_ids', 'ts', 'cand']
    assert sig.parameters['chunk_queries'].default == 65536
