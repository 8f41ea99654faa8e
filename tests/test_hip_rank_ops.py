"""tg_rank_scores and tg_rank_stats called directly (csrc/tg_rank.hip), against the float64 references of
tests/_rank_ref.py on synthetic tensors: no model, no sampler, no oracle state.

Scores.  |got - ref64| <= (2W + d + 8) 2^-24 A per pair (A: the pair's magnitude, _rank_ref.score_ref): the first-order
worst case of the two float32 dot products in any summation order - derived, not tuned.  tests/test_rank_ref_host.py shows
on the reference alone that every term of a score (each 32-column block of y, each hit column, either class table, b1,
the x block) moves some pair by at least 4 bounds, so an off-by-one in `k < W`, `live`, `min(n, d - 1)` or
`min(m0 + tid, P - 1)` cannot hide in the tolerance.  The worst err / bound per case is printed (pytest -s, or the captured
output of a failing case).  Position independence, guard words and the workspace check are bit-exact.

Rank statistics.  Integer outputs equal numpy and the host twin exactly; the float64 sum of 1 / rank within its
summation-order bound B 2^-52 sum(1 / rank).  Shapes take k_rank_event's `j0` loop through 0 .. 3 passes and
k_rank_fold's `i += 64` loop through 1 .. 5."""
import ctypes as C

import numpy as np
import pytest
import torch

from _rank_ref import CASE_IDS, HIT, SCORE_CASES, STATS_SHAPES, case_ref, make_stats_case, numpy_ranks

pytestmark = pytest.mark.gpu
KS8 = (1, 2, 3, 5, 10, 50, 100, 1000)


def dev():
    return torch.device('cuda', 0)


def to_dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def run_scores(c, *, scores=None, ws_short=0):
    """one tg_rank_scores call on the case's arrays -> (return code, scores [B, 1 + C] on the device).  The workspace is
    pre-filled with NaN: the kernel cannot rely on stale contents."""
    from www2023tiger_amd._lib import TgLinear, TgScoreParams, lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    t = {k: to_dev(c[k]) for k in ('h_src', 'h_cand', 'nbr_src', 'nbr_cand', 'src', 'cand_ids', 'w1', 'b1', 'w2', 'b2',
                                   'hit_emb')}
    sp = TgScoreParams(HIT[c['hit']], c['n_hit_rows'], ptr(t['hit_emb']), TgLinear(ptr(t['w1']), ptr(t['b1'])),
                       TgLinear(ptr(t['w2']), ptr(t['b2'])))
    B, C1, d, K = c['B'], c['C'] + 1, c['d'], c['K']
    need = int(lib.tg_rank_scores_workspace_bytes(B, d, C.byref(sp)))
    rows = B + (2 * c['n_hit_rows'] if c['hit'] in ('bin', 'count') else 0)
    assert need >= rows * d * 4
    ws = torch.full(((need + 3) // 4,), float('nan'), dtype=torch.float32, device=dev())
    if scores is None:
        scores = torch.full((B, C1), float('nan'), dtype=torch.float32, device=dev())
    rc = lib.tg_rank_scores(B, C1 - 1, d, K, C.byref(sp), ptr(t['h_src']), ptr(t['h_cand']), ptr(t['nbr_src']),
                            ptr(t['nbr_cand']), ptr(t['src']), ptr(t['cand_ids']), ptr(scores), ptr(ws), need - ws_short,
                            stream_ptr(dev()))
    torch.cuda.synchronize()
    return rc, scores


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize('key', SCORE_CASES, ids=CASE_IDS)
def test_scores_within_the_derived_bound_of_float64(key, request):
    c, ref, bound = case_ref(key)
    rc, got = run_scores(c)
    assert rc == 0
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    ratio = np.abs(got - ref) / bound
    worst = float(ratio.max())
    print(f'{request.node.callspec.id}: worst err / bound {worst:.3e} (err {np.abs(got - ref).max():.2e}, '
          f'pair {int(ratio.argmax())} of {ratio.size})')
    assert worst <= 1.0, (worst, int(ratio.argmax()))


def permuted(c):
    """the events reversed, every event's 1 + C pair columns rolled by 3"""
    q = dict(c)
    for k in ('h_src', 'nbr_src', 'src'):
        q[k] = np.ascontiguousarray(c[k][::-1])
    for k in ('h_cand', 'nbr_cand', 'cand_ids'):
        q[k] = np.ascontiguousarray(np.roll(c[k][::-1], 3, axis=1))
    return q


def single(c, i, j):
    """pair (i, j) as a call of its own: B = 1, C = 0"""
    q = dict(c, B=1, C=0, P=1)
    for k in ('h_src', 'nbr_src', 'src'):
        q[k] = np.ascontiguousarray(c[k][i:i + 1])
    for k in ('h_cand', 'nbr_cand', 'cand_ids'):
        q[k] = np.ascontiguousarray(c[k][i:i + 1, j:j + 1])
    return q


@pytest.mark.parametrize('key,pair', [((32, 16, 3, 10, 'vec'), (1, 9)), ((129, 3, 3, 40, 'count'), (2, 40))],
                         ids=['d32-vec', 'd129-count'])
def test_a_score_does_not_depend_on_its_position_bit_for_bit(key, pair):
    """the same pairs in other tile rows, other tiles and other blocks (the `p / C1` event index, ev[] / cls[] of the
    tile, the repeated rows of a short last tile): equal bits"""
    c, _, _ = case_ref(key)
    rc, base = run_scores(c)
    assert rc == 0
    rc, perm = run_scores(permuted(c))
    assert rc == 0
    back = np.roll(bits(perm), -3, axis=1)[::-1]
    np.testing.assert_array_equal(back, bits(base))
    i, j = pair
    rc, one = run_scores(single(c, i, j))
    assert rc == 0 and one.shape == (1, 1)
    assert bits(one)[0, 0] == bits(base)[i, j]
    assert len(np.unique(bits(base))) == base.numel()   # (no two pairs of the case are alike: the check can tell them apart)


@pytest.mark.parametrize('key', [(30, 2, 4, 7, 'vec'), (33, 5, 31, 0, 'count'), (129, 3, 3, 40, 'count')],
                         ids=['P32', 'P31', 'P123'])
def test_nothing_outside_the_scores_is_written(key):
    """scores pre-filled with NaN inside one allocation with 64 guard floats on either side: every score is written
    (finite), the guards keep their bits (`m0 + tid < P`)"""
    c, ref, bound = case_ref(key)
    P = c['P']
    buf = torch.full((64 + P + 64,), float('nan'), dtype=torch.float32, device=dev())
    guard = torch.arange(1, 129, dtype=torch.float32, device=dev()) * 0.5
    buf[:64], buf[64 + P:] = guard[:64], guard[64:]
    rc, _ = run_scores(c, scores=buf[64:64 + P])
    assert rc == 0
    out = buf.cpu().numpy()
    assert np.isfinite(out[64:64 + P]).all()
    np.testing.assert_array_equal(out[:64].view(np.uint32), guard[:64].cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(out[64 + P:].view(np.uint32), guard[64:].cpu().numpy().view(np.uint32))
    assert (np.abs(out[64:64 + P].astype(np.float64) - ref.reshape(-1)) <= bound.reshape(-1)).all()


def test_a_workspace_one_byte_short_is_refused():
    from www2023tiger_amd._lib import TG_EWORKSPACE
    c, _, _ = case_ref((8, 5, 3, 1, 'bin'))
    rc, scores = run_scores(c, ws_short=1)   # an argument check: nothing is launched
    assert rc == TG_EWORKSPACE
    assert np.isnan(scores.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------ rank statistics
def device_stats(s, ids, dst, mask, ks, acc=None):
    from www2023tiger_amd import hip_ops
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev())
    return hip_ops.rank_stats(t(s), t(ids), t(dst), mask=t(mask), ks=ks, acc=acc)


def host_stats(s, ids, dst, mask, ks):
    from www2023tiger_amd import hip_ops
    t = lambda a: None if a is None else torch.from_numpy(a)
    return hip_ops.rank_stats(t(s), t(ids), t(dst), mask=t(mask), ks=ks)


def assert_counts(st, want):
    g, e, v, r = want
    for k, w in zip(('n_greater', 'n_equal', 'n_valid', 'rank'), (g, e, v, r)):
        np.testing.assert_array_equal(st[k].cpu().numpy(), w, err_msg=k)


def assert_acc(acc, rank, ks, n_events):
    f, i = acc[0].cpu().numpy(), acc[1].cpu().numpy()
    inv = float(np.sum(1.0 / rank))
    assert abs(f[0] - inv) <= len(rank) * 2.0 ** -52 * inv, (f[0], inv)
    for q, k in enumerate(ks):
        assert f[1 + q] == float(np.sum(rank <= k)), (k, f[1 + q])   # integer-valued doubles: exact
    assert (f[1 + len(ks):] == 0).all()
    assert i[0] == n_events and i[1] == 0


@pytest.mark.parametrize('with_mask', [False, True], ids=['no-mask', 'mask'])
@pytest.mark.parametrize('B,C', STATS_SHAPES, ids=[f'B{b}-C{c}' for b, c in STATS_SHAPES])
def test_stats_equal_numpy_and_the_host_twin(B, C, with_mask):
    s, ids, dst, mask = make_stats_case(B, C)
    mask = mask if with_mask else None
    want = numpy_ranks(s, ids, dst, mask)
    if B >= 3:
        assert want[2][B // 2] == 0 and want[3][B // 2] == 1.0   # the event with everything left out
    if C >= 63:
        assert (want[1] > 0).any() and (want[2] < C).all()       # ties; something is left out of every event
    st = device_stats(s, ids, dst, mask, KS8)
    assert st['rank'].dtype == torch.float64 and st['n_greater'].dtype == torch.int32
    assert_counts(st, want)
    assert_acc(st['acc'], want[3], KS8, B)
    h = host_stats(s, ids, dst, mask, KS8)
    for k in ('n_greater', 'n_equal', 'n_valid', 'rank'):
        assert torch.equal(h[k], st[k].cpu()), k
    assert torch.equal(h['acc'][0][1:], st['acc'][0][1:].cpu()) and torch.equal(h['acc'][1], st['acc'][1].cpu())


def test_no_cut_offs_leave_the_hit_sums_alone():
    """n_ks = 0: only acc_f64[0] and the event count move - the accumulator is pre-filled with sentinels"""
    from www2023tiger_amd import _lib
    s, ids, dst, mask = make_stats_case(65, 5)
    f = torch.arange(100, 100 + 1 + _lib.TG_RANK_MAX_K, dtype=torch.float64, device=dev())
    i = torch.tensor([1000, 0], dtype=torch.int64, device=dev())
    st = device_stats(s, ids, dst, mask, (), acc=(f, i))
    want = numpy_ranks(s, ids, dst, mask)
    assert_counts(st, want)
    got = f.cpu().numpy()
    inv = float(np.sum(1.0 / want[3]))
    assert abs(got[0] - (100.0 + inv)) <= 65 * 2.0 ** -52 * (100.0 + inv)
    np.testing.assert_array_equal(got[1:], np.arange(101, 101 + _lib.TG_RANK_MAX_K, dtype=np.float64))
    assert i.cpu().tolist() == [1065, 0]


def test_eight_cut_offs():
    from www2023tiger_amd import _lib, hip_ops
    assert len(KS8) == _lib.TG_RANK_MAX_K
    s, ids, dst, mask = make_stats_case(257, 70)
    st = device_stats(s, ids, dst, None, KS8)
    r = numpy_ranks(s, ids, dst, None)[3]
    m = hip_ops.rank_metrics(st['acc'], KS8)
    assert m['n_events'] == 257 and len({m['hits'][k] for k in KS8}) >= 3   # the cut-offs tell ranks apart
    for k in KS8:
        assert m['hits'][k] == float(np.sum(r <= k)) / 257
    assert m['hits'][100] == m['hits'][1000] == 1.0


def test_the_accumulator_folds_over_device_calls():
    """(130, 3) as calls of 64, 1 and 65 events on one accumulator: the ranks and hit sums of one call"""
    from www2023tiger_amd import hip_ops
    s, ids, dst, mask = make_stats_case(130, 3)
    ks = (1, 2, 3)
    whole = device_stats(s, ids, dst, mask, ks)
    acc = hip_ops.new_rank_acc(dev())
    ranks = []
    for lo, hi in ((0, 64), (64, 65), (65, 130)):
        part = device_stats(s[lo:hi], ids[lo:hi], dst[lo:hi], mask[lo:hi], ks, acc=acc)
        assert part['acc'] is acc
        ranks.append(part['rank'])
    assert torch.equal(torch.cat(ranks), whole['rank'])
    want = numpy_ranks(s, ids, dst, mask)[3]
    np.testing.assert_array_equal(whole['rank'].cpu().numpy(), want)
    assert torch.equal(acc[0][1:], whole['acc'][0][1:]) and torch.equal(acc[1], whole['acc'][1])
    assert_acc(acc, want, ks, 130)
    assert_acc(whole['acc'], want, ks, 130)


def test_non_finite_scores_are_counted_on_the_device():
    from www2023tiger_amd import hip_ops
    B, C = 5, 129
    s, ids, dst, _ = make_stats_case(B, C)
    ids[:, 1:] = 600 + np.arange(C)            # every candidate left in ...
    ids[3, 10] = 0                             # ... but one
    clean = device_stats(s, ids, dst, None, KS8)
    assert int(clean['acc'][1][1]) == 0
    s = s.copy()
    s[0, 1 + 20] = np.nan                      # a candidate left in, first 64-lane pass
    s[1, 0] = np.inf                           # a positive
    s[2, 1 + 100] = -np.inf                    # a candidate left in, second pass
    s[3, 10] = np.nan                          # a candidate left out: not ranked, not counted
    st = device_stats(s, ids, dst, None, KS8)
    assert st['acc'][1].cpu().tolist() == [B, 3]
    with pytest.raises(ValueError, match='3 non-finite'):
        hip_ops.rank_metrics(st['acc'], KS8)
    assert_counts(st, numpy_ranks(s, ids, dst, None))
    for k in ('n_greater', 'n_equal', 'n_valid', 'rank'):   # the untouched events
        assert torch.equal(st[k][3:], clean[k][3:]), k
