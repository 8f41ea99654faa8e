"""Constructed cases of the shared-catalogue score head (include/tiger_hip.h: tg_rank_cand_half, tg_rank_scores_shared),
shared by tests/test_shared_rank_ref_host.py (reference only, no GPU) and tests/test_hip_shared_rank_ops.py (the kernels).

A shared case (d, K, B, C, hit) holds B sources and C items; pair (i, j) is (src[i], cat_ids[j]).  Its reference is
_rank_ref.score_ref on the BROADCAST arrays - h_cand[i, j] = h_cat[j], nbr_cand[i, j] = nbr_cat[j], cand_ids[i, j] =
cat_ids[j], column 0 being item 0 - and its tolerance _rank_ref.score_bound: the shared kernels have no reference of
their own to drift towards."""
import numpy as np

from _rank_ref import REF_ARGS, score_bound, score_ref

# (d, K, B, C, hit): each the smallest shape that reaches its path
SHARED_CASES = [
    (8, 5, 3, 2, 'bin'),        # the smallest
    (8, 6, 1, 1, 'vec'),        # one pair
    (30, 2, 4, 8, 'vec'),       # the hit columns cross a 32-column operand tile; 32 pairs exactly
    (32, 16, 3, 11, 'vec'),     # 33 pairs
    (33, 5, 31, 1, 'count'),    # wave slot 1 holds one column; C = 1
    (96, 4, 5, 7, 'bin'),       # slot 3 dead
    (128, 4, 33, 2, 'none'),    # one full column pass; id arrays NULL
    (129, 3, 3, 41, 'count'),   # second pass holds one column
    (172, 10, 7, 6, 'vec'),     # the project's headline width
    (172, 10, 7, 6, 'count'),   # the project's headline width; n_hit_rows = K + 3 > K + 1 (EXTRA_HIT_ROWS)
    (16, 3, 70, 67, 'bin'),     # B and C beyond 64, neither a multiple of 32
    (16, 4, 65, 1, 'vec'),      # many sources, one item
    # the edges of k_shared_pairs's tile (csrc/tg_rank_snapshot.hip: 16 sources x chunks of 8 items, strips of 64 items) and of
    # the 32-row tile of the half products, on both axes
    (8, 2, 16, 8, 'count'),     # one block, one chunk, every row and column live
    (8, 2, 17, 9, 'bin'),       # one source and one item past: a second block row with one live source, a chunk of one item
    (8, 2, 15, 7, 'none'),      # one short of either: the last tile row has a live source in one half only
    (8, 2, 2, 64, 'bin'),       # one strip exactly (eight full chunks)
    (8, 2, 2, 65, 'count'),     # a second strip of one item
    (8, 2, 1, 63, 'bin'),       # B = 1: the fk = 1 half of every wavefront has no source; a strip one item short
    (8, 2, 3, 32, 'bin'),       # C = 32: one full tile of tg_rank_cand_half
    (8, 2, 1, 33, 'none'),      # C = 33: its second tile holds one item
]
EXTRA_HIT_ROWS = {(172, 10, 7, 6, 'count'): 2}
CASE_IDS = ['d{}-K{}-B{}-C{}-{}'.format(*c) for c in SHARED_CASES]


def make_shared_case(d, K, B, C, hit, seed=0, extra_hit_rows=0):
    """Inputs of tg_rank_cand_half / tg_rank_scores_shared as float32 / int64 numpy arrays; weights with the scales of
    _rank_ref.make_case.  src = 1000 + arange(B), cat_ids = 2000 + arange(C).  Neighbour ids are constructed:
      nbr_cat[j, :] (the sources an item lists; src hits of pair (i, j) = slots equal to src[i]): the last item lists
      src[B - 1] K times.  Item j < C - 1 gives n_j = 1 + j mod (K - 1) random slots to source a_j = 1 + j mod (B - 1) and
      the other K - n_j to the next source, so the pairs (a_j, j) and (a_j + 1, j) get the classes n_j and K - n_j.
      nbr_src[i, :] (the items a source lists; dst hits = slots equal to cat_ids[j]): the same with the roles swapped.
    Pair (B - 1, C - 1) so has all K hits on either side; pair (0, 0) none (source 0 and item 0 are never dealt to in row 0:
    where the rule above would, the foreign ids 7 / 9 stand instead).  A slot that does not hit for the pair it was dealt
    for holds ANOTHER source's / item's id, so a wrong row index hits."""
    rs = np.random.RandomState(1000 * d + 10 * K + B + C + seed + 5)
    W = d + (K if hit == 'vec' else 0)
    f4 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    c = dict(d=d, K=K, B=B, C=C, hit=hit, W=W, P=B * C)
    c['h_src'] = f4(rs.standard_normal((B, d)))
    c['h_cat'] = f4(rs.standard_normal((C, d)))
    w1 = rs.standard_normal((d, 2 * W)) / np.sqrt(2 * W)
    if hit == 'vec':
        w1[:, d:W] = rs.standard_normal((d, K)) * 0.75
        w1[:, W + d:] = rs.standard_normal((d, K)) * 0.75
    c['w1'], c['b1'] = f4(w1), f4(rs.standard_normal(d) * 0.5)
    c['w2'], c['b2'] = f4(rs.standard_normal((1, d)) / np.sqrt(d)), f4([0.25])
    c['n_hit_rows'] = {'bin': 2, 'count': K + 1 + extra_hit_rows}.get(hit, 0)
    c['hit_emb'] = f4(rs.standard_normal((c['n_hit_rows'], d)) * 0.75) if c['n_hit_rows'] else None
    src = 1000 + np.arange(B, dtype=np.int64)
    cat = 2000 + np.arange(C, dtype=np.int64)

    def deal(rows, others, foreign):
        """[len(rows), K] lists over the ids `others`; row r is a row of `rows` (items when others are the sources)"""
        R, O = len(rows), len(others)
        out = np.full((R, K), foreign, dtype=np.int64)
        for r in range(R):
            if r == R - 1:
                out[r, :] = others[O - 1]
                continue
            if O == 1:
                a, fill = 0, foreign
                n = 0 if r == 0 else (1 + r % (K - 1) if K > 1 else 0)
            else:
                a = 1 + r % (O - 1)
                nxt = (a + 1) % O
                fill = foreign if (nxt == 0 and r == 0) else others[nxt]
                n = 1 + r % (K - 1) if K > 1 else 0
            out[r, :] = fill
            out[r, rs.permutation(K)[:n]] = others[a]
        return out
    c['nbr_cat'] = deal(cat, src, 7)
    c['nbr_src'] = deal(src, cat, 9)
    c.update(src=src, cat_ids=cat)
    if hit == 'none':
        c.update(src=None, cat_ids=None, nbr_src=None, nbr_cat=None)
    return c


def broadcast(c):
    """the per-pair form of a shared case: the arguments of _rank_ref.score_ref and of tg_rank_scores with C - 1
    candidate columns behind column 0 (item 0)"""
    B, C, d, K = c['B'], c['C'], c['d'], c['K']
    q = dict(c, C=C - 1)
    q['h_cand'] = np.ascontiguousarray(np.broadcast_to(c['h_cat'][None], (B, C, d)))
    if c['hit'] == 'none':
        q.update(nbr_cand=None, cand_ids=None)
    else:
        q['nbr_cand'] = np.ascontiguousarray(np.broadcast_to(c['nbr_cat'][None], (B, C, K)))
        q['cand_ids'] = np.ascontiguousarray(np.broadcast_to(c['cat_ids'][None], (B, C)))
    return q


_REF = {}


def shared_ref(key):
    """(case, its broadcast form, float64 scores [B, C], bound per pair) of SHARED_CASES entry `key`, computed once and
    left unchanged"""
    if key not in _REF:
        c = make_shared_case(*key, extra_hit_rows=EXTRA_HIT_ROWS.get(key, 0))
        q = broadcast(c)
        s, A = score_ref(*[q[k] for k in REF_ARGS])
        for a in (s, A):
            a.setflags(write=False)
        _REF[key] = (c, q, s, score_bound(A, c['d'], c['W']))
    return _REF[key]
