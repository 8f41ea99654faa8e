"""tg_rank_cand_half and tg_rank_scores_shared called directly (csrc/tg_rank_snapshot.hip) on the constructed cases of
tests/_shared_rank_ref.py: no model, no sampler.

The main claim is exact: a pair's bits equal those of tg_rank_scores on the BROADCAST inputs (every source meets the
same C items), for every shape.  Beside it the scores lie within the derived bound of the float64 reference
(_rank_ref.score_bound; tests/test_shared_rank_ref_host.py shows that every term of a score moves some pair by at least 4
bounds); the worst err / bound per case is printed (pytest -s).  Position independence, leading dimension, guard words
and the workspace check are bit-exact.  Every call runs on a NaN-filled workspace."""
import ctypes as C

import numpy as np
import pytest
import torch

from _rank_ref import HIT
from _shared_rank_ref import CASE_IDS, SHARED_CASES, shared_ref
from test_hip_rank_ops import bits, dev, run_scores, to_dev

pytestmark = pytest.mark.gpu


def params(c, t):
    from www2023tiger_amd._lib import TgLinear, TgScoreParams, ptr
    return TgScoreParams(HIT[c['hit']], c['n_hit_rows'], ptr(t['hit_emb']), TgLinear(ptr(t['w1']), ptr(t['b1'])),
                         TgLinear(ptr(t['w2']), ptr(t['b2'])))


def run_half(c, *, out=None):
    """one tg_rank_cand_half call -> (return code, P [C, d] on the device, pre-filled with NaN)"""
    from www2023tiger_amd._lib import lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    t = {k: to_dev(c[k]) for k in ('h_cat', 'w1', 'b1', 'w2', 'b2', 'hit_emb')}
    sp = params(c, t)
    if out is None:
        out = torch.full((c['C'], c['d']), float('nan'), dtype=torch.float32, device=dev())
    rc = lib.tg_rank_cand_half(c['C'], c['d'], c['K'], C.byref(sp), ptr(t['h_cat']), ptr(out), stream_ptr(dev()))
    torch.cuda.synchronize()
    return rc, out


def run_shared(c, P=None, *, scores=None, ld=None, ws_short=0):
    """tg_rank_cand_half (unless P is given), then one tg_rank_scores_shared call -> (return code, scores [B, ld]).  The
    workspace is pre-filled with NaN: the kernels cannot rely on stale contents."""
    from www2023tiger_amd._lib import lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    if P is None:
        rc, P = run_half(c)
        assert rc == 0
    t = {k: to_dev(c[k]) for k in ('h_src', 'nbr_src', 'nbr_cat', 'src', 'cat_ids', 'w1', 'b1', 'w2', 'b2', 'hit_emb')}
    sp = params(c, t)
    B, Cn, d, K = c['B'], c['C'], c['d'], c['K']
    ld = Cn if ld is None else ld
    need = int(lib.tg_rank_scores_shared_workspace_bytes(B, d, C.byref(sp)))
    rows = B + (2 * c['n_hit_rows'] if c['hit'] in ('bin', 'count') else 0)
    assert need >= rows * d * 4
    ws = torch.full(((need + 3) // 4,), float('nan'), dtype=torch.float32, device=dev())
    if scores is None:
        scores = torch.full((B, ld), float('nan'), dtype=torch.float32, device=dev())
    rc = lib.tg_rank_scores_shared(B, Cn, d, K, C.byref(sp), ptr(t['h_src']), ptr(P), ptr(t['nbr_src']), ptr(t['nbr_cat']),
                                   ptr(t['src']), ptr(t['cat_ids']), ptr(scores), ld, ptr(ws), need - ws_short,
                                   stream_ptr(dev()))
    torch.cuda.synchronize()
    return rc, scores


# ------------------------------------------------------------------------------------------ the main claim
@pytest.mark.parametrize('key', SHARED_CASES, ids=CASE_IDS)
def test_bits_equal_tg_rank_scores_on_the_broadcast_inputs(key):
    c, q, _, _ = shared_ref(key)
    rc, want = run_scores(q)                 # tg_rank_scores: [B, 1 + (C - 1)], every pair row with its own copy
    assert rc == 0 and want.shape == (c['B'], c['C'])
    rc, got = run_shared(c)
    assert rc == 0
    assert np.isfinite(got.cpu().numpy()).all()
    np.testing.assert_array_equal(bits(got), bits(want))


@pytest.mark.parametrize('key', SHARED_CASES, ids=CASE_IDS)
def test_scores_within_the_derived_bound_of_float64(key, request):
    c, _, ref, bound = shared_ref(key)
    rc, got = run_shared(c)
    assert rc == 0
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    ratio = np.abs(got - ref) / bound
    worst = float(ratio.max())
    print(f'{request.node.callspec.id}: worst err / bound {worst:.3e} (err {np.abs(got - ref).max():.2e}, '
          f'pair {int(ratio.argmax())} of {ratio.size})')
    assert worst <= 1.0, (worst, int(ratio.argmax()))


# ------------------------------------------------------------------------------------------ position independence
POS_KEYS = [(32, 16, 3, 11, 'vec'), (129, 3, 3, 41, 'count'), (16, 3, 70, 67, 'bin'), (128, 4, 33, 2, 'none')]
POS_IDS = ['d32-vec', 'd129-count', 'd16-bin-B70-C67', 'd128-none']


def permuted(c, rs):
    """(the case with its sources and its items shuffled, the two permutations)"""
    pi, pj = rs.permutation(c['B']), rs.permutation(c['C'])
    q = dict(c)
    for k in ('h_src', 'nbr_src', 'src'):
        q[k] = None if c[k] is None else np.ascontiguousarray(c[k][pi])
    for k in ('h_cat', 'nbr_cat', 'cat_ids'):
        q[k] = None if c[k] is None else np.ascontiguousarray(c[k][pj])
    return q, pi, pj


@pytest.mark.parametrize('key', POS_KEYS, ids=POS_IDS)
def test_a_row_of_P_does_not_depend_on_its_position(key):
    """the catalogue rows shuffled: the same bits, shuffled (other tile rows, other tiles, the repeated rows of a short
    last tile)"""
    c, _, _, _ = shared_ref(key)
    rc, base = run_half(c)
    assert rc == 0 and np.isfinite(base.cpu().numpy()).all()
    q, _, pj = permuted(c, np.random.RandomState(3))
    rc, perm = run_half(q)
    assert rc == 0
    np.testing.assert_array_equal(bits(perm), bits(base)[pj])
    assert len(np.unique(bits(base), axis=0)) == c['C']   # (no two rows are alike: the check can tell them apart)


@pytest.mark.parametrize('key', POS_KEYS, ids=POS_IDS)
def test_a_score_does_not_depend_on_its_position(key):
    """sources and items shuffled: the same score bits, shuffled; and the last pair and a middle one as B = 1, C = 1 calls"""
    c, _, _, _ = shared_ref(key)
    rc, base = run_shared(c)
    assert rc == 0
    q, pi, pj = permuted(c, np.random.RandomState(4))
    rc, perm = run_shared(q)
    assert rc == 0
    np.testing.assert_array_equal(bits(perm), bits(base)[pi][:, pj])
    assert len(np.unique(bits(base))) >= base.numel() - 1 - (c['hit'] == 'none')   # pairs differ: the check can tell them apart
    for i, j in ((c['B'] - 1, c['C'] - 1), (c['B'] // 2, c['C'] // 2)):
        one = dict(c, B=1, C=1, P=1)
        for k in ('h_src', 'nbr_src', 'src'):
            one[k] = None if c[k] is None else np.ascontiguousarray(c[k][i:i + 1])
        for k in ('h_cat', 'nbr_cat', 'cat_ids'):
            one[k] = None if c[k] is None else np.ascontiguousarray(c[k][j:j + 1])
        rc, s = run_shared(one)
        assert rc == 0 and s.shape == (1, 1)
        assert bits(s)[0, 0] == bits(base)[i, j], (i, j)


# ------------------------------------------------------------------------------------------ nothing else is written
GUARD_KEYS = [(30, 2, 4, 8, 'vec'), (33, 5, 31, 1, 'count'), (8, 2, 17, 9, 'bin'), (8, 2, 1, 63, 'bin'), (8, 2, 1, 33, 'none')]


@pytest.mark.parametrize('key', GUARD_KEYS, ids=['d{}-K{}-B{}-C{}-{}'.format(*k) for k in GUARD_KEYS])
def test_a_wider_leading_dimension_and_guard_words(key):
    """scores [B, ld] with ld = C + 5 inside one allocation with 64 guard floats on either side: every score is written and
    equals the dense call's bits, the NaN behind every row and the guards keep theirs; the same guards around P"""
    c, _, _, _ = shared_ref(key)
    B, Cn, d = c['B'], c['C'], c['d']
    rc, dense = run_shared(c)
    assert rc == 0
    ld = Cn + 5
    guard = torch.arange(1, 129, dtype=torch.float32, device=dev()) * 0.5
    buf = torch.full((64 + B * ld + 64,), float('nan'), dtype=torch.float32, device=dev())
    buf[:64], buf[64 + B * ld:] = guard[:64], guard[64:]
    rc, _ = run_shared(c, scores=buf[64:64 + B * ld].view(B, ld), ld=ld)
    assert rc == 0
    out = buf.cpu().numpy()
    body = out[64:64 + B * ld].reshape(B, ld)
    np.testing.assert_array_equal(body[:, :Cn].view(np.uint32), bits(dense))
    assert np.isnan(body[:, Cn:]).all()
    g = guard.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(out[:64].view(np.uint32), g[:64])
    np.testing.assert_array_equal(out[64 + B * ld:].view(np.uint32), g[64:])
    pbuf = torch.full((64 + Cn * d + 64,), float('nan'), dtype=torch.float32, device=dev())
    pbuf[:64], pbuf[64 + Cn * d:] = guard[:64], guard[64:]
    rc, P = run_half(c, out=pbuf[64:64 + Cn * d].view(Cn, d))
    assert rc == 0
    pout = pbuf.cpu().numpy()
    assert np.isfinite(pout[64:64 + Cn * d]).all()
    np.testing.assert_array_equal(pout[:64].view(np.uint32), g[:64])
    np.testing.assert_array_equal(pout[64 + Cn * d:].view(np.uint32), g[64:])
    rc, again = run_half(c)
    np.testing.assert_array_equal(bits(P), bits(again))


def test_P_is_the_candidate_half_within_its_bound():
    """P[j, n] = sum_k W1[n, W + k] h_cat[j, k] against float64: |err| <= d 2^-24 sum_k |w| |h| (any summation order)"""
    for key in ((172, 10, 7, 6, 'vec'), (33, 5, 31, 1, 'count')):
        c, _, _, _ = shared_ref(key)
        rc, P = run_half(c)
        assert rc == 0
        d, W = c['d'], c['W']
        w = c['w1'][:, W:W + d].astype(np.float64)
        h = c['h_cat'].astype(np.float64)
        ref, mag = h @ w.T, np.abs(h) @ np.abs(w).T
        err = np.abs(P.cpu().numpy().astype(np.float64) - ref)
        assert (err <= d * 2.0 ** -24 * mag).all(), float((err / mag).max())
        assert (np.abs(ref) > 0.05).mean() > 0.5   # (not a matrix of zeros)


# ------------------------------------------------------------------------------------------ refusals on the device
def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    from www2023tiger_amd._lib import TG_EINVAL
    c, _, _, _ = shared_ref((8, 5, 3, 2, 'bin'))
    rc, scores = run_shared(c, ws_short=1)   # an argument check: nothing is launched
    assert rc == TG_EINVAL
    assert np.isnan(scores.cpu().numpy()).all()


def test_vec_hits_with_an_odd_width_are_unsupported():
    from www2023tiger_amd._lib import TG_EUNSUPPORTED
    from _shared_rank_ref import make_shared_case
    c = make_shared_case(7, 5, 2, 3, 'vec')   # 2 (d + K) = 24 is aligned: the odd d alone refuses
    rc, P = run_half(c)
    assert rc == TG_EUNSUPPORTED and np.isnan(P.cpu().numpy()).all()
    rc, scores = run_shared(c, P=P)
    assert rc == TG_EUNSUPPORTED and np.isnan(scores.cpu().numpy()).all()
