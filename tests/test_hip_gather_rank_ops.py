"""tg_rank_scores_gathered called directly (csrc/tg_rank_snapshot.hip) on the constructed cases of tests/_shared_rank_ref.py:
no model, no sampler.  Two yardsticks per call, and no pair is left out of either:

  exact   for col[i, q] = j >= 0 the bits of tg_rank_scores_shared at [i, j] on the same inputs (the order contract is
          inherited: tests/test_hip_shared_rank_ops.py ties those bits to tg_rank_scores on the broadcast inputs); for
          col[i, q] < 0 the value 0.0 exactly;
  float64 within _rank_ref.score_bound of the float64 score s[i, j] - so the two kernels cannot drift together.

The col patterns stand at the edges of the NEW kernel's tile (k_gather_pairs: one source per block, chunks of GA_CH = 16
columns - the fk halves of a wavefront take alternate items - and strips of GA_JS = 32; k_snap_vec<true>: 32 pair rows).  Every
call runs on a NaN-filled workspace and a NaN-filled score array."""
import ctypes as C

import numpy as np
import pytest
import torch

from _shared_rank_ref import make_shared_case, shared_ref
from test_hip_rank_ops import bits, dev, to_dev
from test_hip_shared_rank_ops import params, run_half, run_shared

pytestmark = pytest.mark.gpu
GA_CH, GA_JS = 16, 32   # csrc/tg_rank_snapshot.hip: columns of a chunk, columns of a block's strip

KEYS = [(8, 5, 3, 2, 'bin'), (8, 6, 1, 1, 'vec'), (30, 2, 4, 8, 'vec'), (33, 5, 31, 1, 'count'), (96, 4, 5, 7, 'bin'),
        (128, 4, 33, 2, 'none'), (129, 3, 3, 41, 'count'), (172, 10, 7, 6, 'vec'), (172, 10, 7, 6, 'count'),
        (16, 3, 70, 67, 'bin'), (8, 2, 1, 63, 'bin')]
KEY_IDS = ['d{}-K{}-B{}-C{}-{}'.format(*k) for k in KEYS]


def run_gathered(c, P, col, *, B=None, Cn=None, scores=None, ld=None, ws_short=0, drop=(), **over):
    """one tg_rank_scores_gathered call on the first B sources of the case -> (return code, scores [B, ld]).  col: int32
    numpy [B, Cq] (None: a NULL pointer).  drop: names of pointer arguments passed as NULL; over: sizes passed as given."""
    from www2023tiger_amd._lib import lib, ptr
    from www2023tiger_amd.hip_ops import stream_ptr
    t = {k: to_dev(c[k]) for k in ('h_src', 'nbr_src', 'nbr_cat', 'src', 'cat_ids', 'w1', 'b1', 'w2', 'b2', 'hit_emb')}
    t['P'] = P
    sp = params(c, {k: (None if k in drop else v) for k, v in t.items()})
    B = c['B'] if B is None else B
    Cn = c['C'] if Cn is None else Cn
    d, K = c['d'], c['K']
    Cq = over.pop('Cq', None if col is None else col.shape[1])
    ld = Cq if ld is None else ld
    need = int(lib.tg_rank_scores_gathered_workspace_bytes(max(B, 0), d, C.byref(sp)))
    assert need == int(lib.tg_rank_scores_shared_workspace_bytes(max(B, 0), d, C.byref(sp)))
    t['ws'] = torch.full(((need + 3) // 4 + 4,), float('nan'), dtype=torch.float32, device=dev())
    t['col'] = None if col is None else to_dev(np.ascontiguousarray(col, dtype=np.int32))
    if scores is None:
        scores = torch.full((max(B, 1), max(ld, 1)), float('nan'), dtype=torch.float32, device=dev())
    t['scores'] = scores
    p = {k: (None if k in drop else ptr(v)) for k, v in t.items()}
    rc = lib.tg_rank_scores_gathered(over.pop('B_arg', B), over.pop('C_arg', Cn), Cq, over.pop('d', d), over.pop('K', K),
                                     None if 'sp' in drop else C.byref(sp), p['h_src'], p['P'], p['nbr_src'], p['nbr_cat'],
                                     p['src'], p['cat_ids'], p['col'], p['scores'], ld, p['ws'], need - ws_short,
                                     stream_ptr(dev()))
    assert not over
    torch.cuda.synchronize()
    return rc, scores


_FULL = {}


def full_of(key):
    """(case, float64 scores [B, C], bound [B, C], P on the device, the bits of tg_rank_scores_shared [B, C]), once per key"""
    if key not in _FULL:
        c, _, s, bound = shared_ref(key)
        rc, P = run_half(c)
        assert rc == 0
        rc, full = run_shared(c, P=P)
        assert rc == 0 and np.isfinite(full.cpu().numpy()).all()
        _FULL[key] = (c, s, bound, P, bits(full))
    return _FULL[key]


def check(key, col, what, B=None):
    """one call on `col` against both yardsticks -> the worst err / bound over the pairs with col >= 0"""
    c, s, bound, P, full = full_of(key)
    col = np.ascontiguousarray(col, dtype=np.int32)
    B = c['B'] if B is None else B
    assert col.shape[0] == B and col.max(initial=-1) < c['C']
    rc, got = run_gathered(c, P, col, B=B)
    assert rc == 0, what
    got = got.cpu().numpy()
    assert got.shape == col.shape, what
    rows = np.arange(B)[:, None]
    inside = col >= 0
    want = np.where(inside, full[rows, np.maximum(col, 0)], np.uint32(0))   # 0.0f is the word 0: -0.0 would not pass
    np.testing.assert_array_equal(got.view(np.uint32), want, err_msg=what)
    ratio = np.abs(got.astype(np.float64) - s[rows, np.maximum(col, 0)]) / bound[rows, np.maximum(col, 0)]
    worst = float(np.where(inside, ratio, 0.0).max(initial=0.0))
    assert worst <= 1.0, (what, worst)
    return worst


def patterns(key):
    """(name, col [B', Cq], B') for a key: every pattern of the module's docstring"""
    d, K, B, Cn, hit = key
    rs = np.random.RandomState(d + 7 * K + B + Cn)
    out = [('identity', np.tile(np.arange(Cn), (B, 1)), B), ('reversed', np.tile(np.arange(Cn)[::-1], (B, 1)), B)]
    for Cq in (1, 2, GA_CH - 1, GA_CH, GA_CH + 1, GA_JS, GA_JS + 1):
        out.append((f'random with repeats, Cq = {Cq}', rs.randint(0, Cn, (B, Cq)), B))
    # about a quarter -1; at least half of every array >= 0
    Cq = 2 * GA_CH + 3
    col = rs.randint(0, Cn, (B, Cq))
    col[rs.rand(B, Cq) < 0.25] = -1
    if (col >= 0).sum() * 2 < col.size:
        col[:, ::2] = np.maximum(col[:, ::2], 0)
    assert (col >= 0).sum() * 2 >= col.size
    out.append(('a quarter outside the catalogue', col, B))
    col = rs.randint(0, Cn, (B, GA_CH + 3))
    col[B // 2] = -1
    out.append(('one row all -1', col, B))
    out.append(('Cq > C', rs.randint(0, Cn, (B, Cn + 3)), B))
    # B = 1: with one column the fk = 1 half of every wavefront (one tile row of 'vec' but the first) is idle
    for Cq in (1, GA_CH + 1):
        out.append((f'B = 1, Cq = {Cq}', rs.randint(0, Cn, (1, Cq)), 1))
    return out


@pytest.mark.parametrize('key', KEYS, ids=KEY_IDS)
def test_bits_equal_the_shared_kernel_at_col_and_lie_within_the_bound_of_float64(key, request):
    c, _, _, _, full = full_of(key)
    worst, n_pairs = 0.0, 0
    for name, col, B in patterns(key):
        worst = max(worst, check(key, col, name, B))
        n_pairs += col.size
    print(f'{request.node.callspec.id}: {n_pairs} pairs, worst err / bound {worst:.3e}')
    # the identity pattern compared whole arrays; pairs differ, so a wrong row would show
    assert len(np.unique(full)) >= full.size - 1 - (c['hit'] == 'none')


@pytest.mark.parametrize('key', [(30, 2, 4, 8, 'vec'), (129, 3, 3, 41, 'count'), (8, 2, 1, 63, 'bin'), (128, 4, 33, 2, 'none')],
                         ids=['vec', 'count', 'bin-B1', 'none'])
def test_a_wider_leading_dimension_and_guard_words(key):
    """scores [B, ld] with ld = Cq + 5 inside one allocation with 64 guard floats on either side: columns q < Cq are
    written (0.0 where col < 0), the NaN behind every row and the guards survive"""
    c, _, _, P, full = full_of(key)
    B, Cn = c['B'], c['C']
    rs = np.random.RandomState(11)
    Cq = GA_JS + 3
    col = rs.randint(-1, Cn, (B, Cq)).astype(np.int32)
    ld = Cq + 5
    guard = torch.arange(1, 129, dtype=torch.float32, device=dev()) * 0.5
    buf = torch.full((64 + B * ld + 64,), float('nan'), dtype=torch.float32, device=dev())
    buf[:64], buf[64 + B * ld:] = guard[:64], guard[64:]
    rc, _ = run_gathered(c, P, col, scores=buf[64:64 + B * ld].view(B, ld), ld=ld)
    assert rc == 0
    out = buf.cpu().numpy()
    body = out[64:64 + B * ld].reshape(B, ld)
    want = np.where(col >= 0, full[np.arange(B)[:, None], np.maximum(col, 0)], np.uint32(0))
    np.testing.assert_array_equal(body[:, :Cq].view(np.uint32), want)
    assert np.isnan(body[:, Cq:]).all()
    g = guard.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(out[:64].view(np.uint32), g[:64])
    np.testing.assert_array_equal(out[64 + B * ld:].view(np.uint32), g[64:])


def test_an_empty_catalogue_scores_zero_everywhere():
    """C = 0 with Cq > 0: every col is negative, the scores are 0.0; P may be NULL"""
    c, _, _, P, _ = full_of((8, 5, 3, 2, 'bin'))
    col = np.full((3, GA_CH + 1), -1, dtype=np.int32)
    rc, got = run_gathered(c, P, col, Cn=0, ld=GA_CH + 3, drop=('P',))
    assert rc == 0
    got = got.cpu().numpy()
    assert (got[:, :GA_CH + 1].view(np.uint32) == 0).all() and np.isnan(got[:, GA_CH + 1:]).all()


# ------------------------------------------------------------------------------------------ status codes
def test_status_codes_and_nothing_is_written():
    from www2023tiger_amd._lib import TG_EINVAL, TG_EUNSUPPORTED, TG_OK
    key = (8, 5, 3, 2, 'bin')
    c, _, _, P, full = full_of(key)
    col = np.array([[0, 1, -1, 1]] * 3, dtype=np.int32)

    def untouched(rc_want, **kw):
        rc, scores = run_gathered(c, P, kw.pop('col', col), **kw)
        assert rc == rc_want, kw
        assert np.isnan(scores.cpu().numpy()).all(), kw

    for kw in (dict(B_arg=-1), dict(C_arg=-1), dict(Cq=-1), dict(d=0), dict(d=-8), dict(K=-1), dict(ld=3), dict(ws_short=1),
               dict(C_arg=2 ** 31 - 1), dict(B_arg=2 ** 16, Cq=2 ** 15), dict(drop=('sp',)), dict(drop=('w1',)), dict(drop=('b2',)),
               dict(drop=('hit_emb',)), dict(drop=('h_src',)), dict(drop=('P',)), dict(drop=('scores',)), dict(drop=('ws',)),
               dict(drop=('col',)), dict(col=None), dict(drop=('nbr_src',)), dict(drop=('nbr_cat',)), dict(drop=('src',)),
               dict(drop=('cat_ids',)), dict(K=0)):
        if 'Cq' in kw and kw['Cq'] > 0:
            kw['ld'] = kw['Cq']
        elif kw.get('col', col) is None:
            kw.update(Cq=4)
        untouched(TG_EINVAL, **kw)
    few = dict(c, n_hit_rows=1)   # 'bin' needs two class rows
    rc, scores = run_gathered(few, P, col)
    assert rc == TG_EINVAL and np.isnan(scores.cpu().numpy()).all()
    # 'vec': an odd d; 2 (d + K) not a multiple of 4
    for d, K in ((7, 5), (8, 5)):
        v = make_shared_case(d, K, 2, 3, 'vec')
        Pv = torch.full((3, d), float('nan'), dtype=torch.float32, device=dev())
        rc, scores = run_gathered(v, Pv, np.zeros((2, 4), dtype=np.int32))
        assert rc == TG_EUNSUPPORTED and np.isnan(scores.cpu().numpy()).all()
    # nothing to do: TG_OK, the output untouched, no pointer looked at
    untouched(TG_OK, B_arg=0)
    untouched(TG_OK, Cq=0)
    untouched(TG_OK, Cq=0, drop=('col', 'h_src', 'P', 'ws', 'scores'))
    # 'none' takes NULL id arrays
    n, _, _, Pn, fn = full_of((128, 4, 33, 2, 'none'))
    rc, got = run_gathered(n, Pn, np.tile(np.arange(2), (33, 1)))
    assert rc == TG_OK
    np.testing.assert_array_equal(bits(got), fn)
    # and the good call still works after all the refusals
    rc, got = run_gathered(c, P, col)
    assert rc == TG_OK
    np.testing.assert_array_equal(bits(got), np.where(col >= 0, full[np.arange(3)[:, None], np.maximum(col, 0)], 0))
