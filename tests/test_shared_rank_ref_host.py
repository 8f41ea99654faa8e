"""The constructed shared-catalogue cases (tests/_shared_rank_ref.py) without a GPU, on the float64 reference alone - what
tests/test_rank_ref_host.py shows for the per-pair cases: the constructed neighbour lists reach every hit column and class,
and every term of the score moves some pair's reference by at least four times that pair's bound, so a kernel that lost
the term (a wrong source or item row, a dead wavefront's columns, a hit column from the wrong side, P without its
source half) cannot stay inside the derived tolerance of tests/test_hip_shared_rank_ops.py."""
import numpy as np
import pytest

from _rank_ref import REF_ARGS, pair_hits, score_bound, score_ref
from _shared_rank_ref import CASE_IDS, SHARED_CASES, broadcast, make_shared_case, shared_ref
from test_rank_ref_host import terms


def hits_of(c, q):
    sh, dh = pair_hits(q['nbr_src'], q['nbr_cand'], q['src'], q['cand_ids'])   # [B, C, K] each
    return sh, dh


@pytest.mark.parametrize('key', SHARED_CASES, ids=CASE_IDS)
def test_the_case_is_the_broadcast_form_of_its_shared_arrays(key):
    c, q, ref, bound = shared_ref(key)
    d, K, B, C, hit = key
    assert ref.shape == (B, C) == bound.shape and (bound > 0).all()
    assert c['h_cat'].shape == (C, d) and c['h_src'].shape == (B, d) and q['h_cand'].shape == (B, C, d)
    for i in range(B):
        np.testing.assert_array_equal(q['h_cand'][i], c['h_cat'])
    if hit == 'none':
        assert all(c[k] is None for k in ('src', 'cat_ids', 'nbr_src', 'nbr_cat'))
        return
    np.testing.assert_array_equal(c['src'], 1000 + np.arange(B))
    np.testing.assert_array_equal(c['cat_ids'], 2000 + np.arange(C))
    assert c['nbr_cat'].shape == (C, K) and c['nbr_src'].shape == (B, K)
    # the hit definition of the shared entry, said directly, equals that of the broadcast form
    sh, dh = hits_of(c, q)
    np.testing.assert_array_equal(sh, (c['nbr_cat'][None, :, :] == c['src'][:, None, None]).astype(np.float64))
    np.testing.assert_array_equal(dh, (c['nbr_src'][:, None, :] == c['cat_ids'][None, :, None]).astype(np.float64))


@pytest.mark.parametrize('key', [k for k in SHARED_CASES if k[4] != 'none'],
                         ids=[i for i, k in zip(CASE_IDS, SHARED_CASES) if k[4] != 'none'])
def test_constructed_neighbours_reach_every_column_and_class(key):
    c, q, _, _ = shared_ref(key)
    d, K, B, C, hit = key
    sh, dh = hits_of(c, q)
    assert sh.reshape(-1, K).any(0).all() and dh.reshape(-1, K).any(0).all()   # every hit column, either side
    assert sh[B - 1, C - 1].all() and dh[B - 1, C - 1].all()                   # one pair with all K hits on both sides
    if B * C >= 2:
        assert not sh[0, 0].any() and not dh[0, 0].any()                       # and one with none
    # a slot that does not hit for the pair it was dealt for names another source / another item (or, where source 0 /
    # item 0 must stay clear, the foreign ids 7 / 9): a wrong row index hits
    src, cat = set(c['src'].tolist()), set(c['cat_ids'].tolist())
    assert set(c['nbr_cat'].reshape(-1).tolist()) <= src | {7} and set(c['nbr_src'].reshape(-1).tolist()) <= cat | {9}
    if B > 1 and C > 1 and K > 1:   # some list names two different sources / items: the dealt one and another
        assert any(len(set(r.tolist())) == 2 for r in c['nbr_cat']) and any(len(set(r.tolist())) == 2 for r in c['nbr_src'])
    if hit == 'count':
        assert c['n_hit_rows'] >= K + 1
        every = set(range(K + 1))
        # src side: the C - 1 items before the last deal the classes n and (B > 1) K - n, n = 1, 2, ...; dst side likewise
        room_s = C - 1 >= K - 1 or (B > 1 and 2 * (C - 1) >= K - 1)
        room_d = B - 1 >= K - 1 or (C > 1 and 2 * (B - 1) >= K - 1)
        if room_s:
            assert set(sh.sum(2).astype(int).reshape(-1).tolist()) == every
        if room_d:
            assert set(dh.sum(2).astype(int).reshape(-1).tolist()) == every
        assert room_s or room_d
    if hit == 'bin':
        assert c['n_hit_rows'] == 2
    rms = lambda a: float(np.sqrt((a.astype(np.float64) ** 2).mean()))
    if hit in ('bin', 'count'):
        assert rms(c['hit_emb']) >= 0.5
    else:
        W = c['W']
        assert rms(c['w1'][:, d:W]) >= 0.5 and rms(c['w1'][:, W + d:]) >= 0.5


def test_the_count_cases_of_the_headline_width_reach_every_class_on_either_side():
    c, q, _, _ = shared_ref((172, 10, 7, 6, 'count'))
    sh, dh = hits_of(c, q)
    assert set(sh.sum(2).astype(int).reshape(-1).tolist()) == set(range(11)) == set(dh.sum(2).astype(int).reshape(-1).tolist())
    assert c['n_hit_rows'] == 13   # more embedding rows than classes


@pytest.mark.parametrize('key', SHARED_CASES, ids=CASE_IDS)
def test_every_term_moves_a_score_by_four_bounds(key):
    """the terms of tests/test_rank_ref_host.py: each 32-column block of y (here: of P), each hit column, T_s, T_d, b1, x"""
    c, q, ref, bound = shared_ref(key)
    worst = None
    for name, repl in terms(q):
        a = dict(q, **{k: v for k, v in repl.items() if k != 'omit'})
        s, _ = score_ref(*[a[k] for k in REF_ARGS], omit=repl.get('omit', ()))
        moved = float((np.abs(s - ref) / bound).max())
        worst = moved if worst is None else min(worst, moved)
        assert moved >= 4.0, (name, moved)
    print(f'{CASE_IDS[SHARED_CASES.index(key)]}: the least visible term moves a pair by {worst:.0f} bounds')


def test_the_bound_is_that_of_the_per_pair_cases():
    c, q, ref, bound = shared_ref((172, 10, 7, 6, 'vec'))
    _, A = score_ref(*[q[k] for k in REF_ARGS])
    np.testing.assert_array_equal(bound, score_bound(A, 172, 182))
    c2 = make_shared_case(172, 10, 7, 6, 'vec')
    for k in ('h_src', 'h_cat', 'w1', 'nbr_cat', 'nbr_src'):
        np.testing.assert_array_equal(c[k], c2[k])   # a case is a function of its key
    assert broadcast(c2)['C'] == 5
