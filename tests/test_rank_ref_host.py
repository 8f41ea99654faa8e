"""The float64 reference of the ranking score head (tests/_rank_ref.py) without a GPU: against the oracle's own score
head, and the condition that keeps the derived tolerance of tests/test_hip_rank_ops.py honest - in every case, every term
of the score moves some pair's reference by at least four times that pair's bound, so a kernel that lost the term (a wrong
tile index, a dead wavefront's columns, a hit column read from the wrong side) cannot stay inside it."""
import numpy as np
import pytest
import torch

from _rank_ref import CASE_IDS, REF_ARGS, SCORE_CASES, case_ref, make_case, pair_hits, score_bound, score_ref


def oracle_scores(c):
    """oracle/tiger_oracle.py:503-509 restated (torch.cat, the hit embedding indexed by max / sum) in torch.float64, then
    the oracle's own score_fn (merge_layer) - column 0 as its positives, column j >= 1 fed as its negatives"""
    from oracle import tiger_oracle as O
    t = lambda a: torch.from_numpy(np.asarray(a)).to(torch.float64)
    p = {'score_fn.fc1.weight': t(c['w1']), 'score_fn.fc1.bias': t(c['b1']),
         'score_fn.fc2.weight': t(c['w2']), 'score_fn.fc2.bias': t(c['b2'])}
    hit_type = c['hit']
    B, C1 = c['h_cand'].shape[:2]
    if hit_type in ('bin', 'count'):
        p['hit_embedding.weight'] = t(c['hit_emb'])
    out = np.zeros((B, C1))
    x, y = t(c['h_src']), t(c['h_cand'][:, 0])
    for j in range(C1):
        ny = t(c['h_cand'][:, j])
        hits = [None] * 4
        if hit_type != 'none':   # data_loader.py:61-75, restated here (not _rank_ref.pair_hits): the source among the
            # candidate's neighbours, the candidate among the source's
            src_hits = lambda jj: c['nbr_cand'][:, jj, :] == c['src'][:, None]
            dst_hits = lambda jj: c['nbr_src'] == c['cand_ids'][:, jj][:, None]
            hits = [t(src_hits(0)), t(dst_hits(0)), t(src_hits(j)), t(dst_hits(j))]
        if hit_type == 'vec':
            xp, yp, xn, yn = (torch.cat([a, b], 1) for a, b in zip((x, y, x, ny), hits))
        elif hit_type in ('bin', 'count'):
            emb = p['hit_embedding.weight']
            red = (lambda v: v.max(1).values.long()) if hit_type == 'bin' else (lambda v: v.sum(1).long())
            xp, yp, xn, yn = (a + emb[red(b)] for a, b in zip((x, y, x, ny), hits))
        else:
            xp, yp, xn, yn = x, y, x, ny
        ps = O.merge_layer(xp, yp, p, 'score_fn.').squeeze(1)
        ns = O.merge_layer(xn, yn, p, 'score_fn.').squeeze(1)
        assert ps.dtype == torch.float64
        out[:, j] = (ps if j == 0 else ns).numpy()
    return out


@pytest.mark.parametrize('hit', ['none', 'vec', 'bin', 'count'])
def test_reference_equals_the_oracle_score_head(hit):
    for d, K, B, C in ((16, 10, 5, 7), (172, 10, 3, 4)):
        c = make_case(d, K, B, C, hit)
        if hit == 'none':   # the reference ignores the id arrays; the oracle head gets none
            assert c['src'] is None
        got, A = score_ref(*[c[k] for k in REF_ARGS])
        want = oracle_scores(c)
        assert got.shape == want.shape == (B, 1 + C) and (A > 0).all()
        assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), np.abs(got - want).max()
        assert np.abs(got).max() > 0.1


def terms(c):
    """(name, replacement arguments) for every term of the score taken out in turn"""
    d, K, W, hit = c['d'], c['K'], c['W'], c['hit']

    def without(lo, hi):
        w = c['w1'].copy()
        w[:, lo:hi] = 0
        return dict(w1=w)
    out = [(f'y[{lo}:{min(lo + 32, d)}]', without(W + lo, W + min(lo + 32, d))) for lo in range(0, d, 32)]
    if hit == 'vec':
        out += [(f'dst hit column {k}', without(W + d + k, W + d + k + 1)) for k in range(K)]
        out += [(f'src hit column {k}', without(d + k, d + k + 1)) for k in range(K)]
    if hit in ('bin', 'count'):
        out += [('T_s', dict(omit=('T_s',))), ('T_d', dict(omit=('T_d',)))]
    out += [('b1', dict(b1=np.zeros_like(c['b1']))), ('x', without(0, d))]
    return out


@pytest.mark.parametrize('key', SCORE_CASES, ids=CASE_IDS)
def test_every_term_moves_a_score_by_four_bounds(key):
    c, ref, bound = case_ref(key)
    assert ref.shape == (c['B'], c['C'] + 1) and (bound > 0).all()
    worst = None
    for name, repl in terms(c):
        a = dict(c, **{k: v for k, v in repl.items() if k != 'omit'})
        s, _ = score_ref(*[a[k] for k in REF_ARGS], omit=repl.get('omit', ()))
        moved = float((np.abs(s - ref) / bound).max())
        worst = moved if worst is None else min(worst, moved)
        assert moved >= 4.0, (name, moved)
    print(f'{CASE_IDS[SCORE_CASES.index(key)]}: the least visible term moves a pair by {worst:.0f} bounds')


@pytest.mark.parametrize('key', SCORE_CASES, ids=CASE_IDS)
def test_constructed_neighbours_reach_every_column_and_class(key):
    c, _, _ = case_ref(key)
    K, P, hit = c['K'], c['P'], c['hit']
    if hit == 'none':
        assert all(c[k] is None for k in ('src', 'cand_ids', 'nbr_src', 'nbr_cand'))
        return
    sh, dh = pair_hits(c['nbr_src'], c['nbr_cand'], c['src'], c['cand_ids'])
    sh, dh = sh.reshape(P, K), dh.reshape(P, K)
    assert sh.any(0).all() and dh.any(0).all()                       # every hit column, either side
    assert sh[-1].all() and dh[-1].all()                             # the last pair: all K neighbours equal
    if P >= 2:
        assert not sh[0].any() and not dh[0].any()                   # a pair without hits
    if hit == 'count':
        assert c['n_hit_rows'] >= K + 1 and set(sh.sum(1)) == set(range(min(P, K + 1))) | {K}
        assert set(dh.sum(1)) == set(range(K + 1))                   # every class on the dst side too
    if hit == 'bin':
        assert c['n_hit_rows'] == 2
    rms = lambda a: float(np.sqrt((a.astype(np.float64) ** 2).mean()))
    if hit in ('bin', 'count'):
        assert rms(c['hit_emb']) >= 0.5
    else:
        d, W = c['d'], c['W']
        assert rms(c['w1'][:, d:W]) >= 0.5 and rms(c['w1'][:, W + d:]) >= 0.5


def test_one_case_has_more_embedding_rows_than_classes():
    assert sum(1 for k in SCORE_CASES if k[4] == 'count' and case_ref(k)[0]['n_hit_rows'] > k[1] + 1) == 1


def test_the_bound_is_the_derived_one():
    A = np.array([2.0, 3.0])
    np.testing.assert_array_equal(score_bound(A, 172, 182), (2 * 182 + 172 + 8) * 2.0 ** -24 * A)
