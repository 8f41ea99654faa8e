"""Plain float64 references of the ranking evaluation (include/tiger_hip.h, ranking section), and the synthetic cases
that tests/test_rank_ref_host.py (reference only, no GPU) and tests/test_hip_rank_ops.py (the kernels) share.

score_ref     the score head in the concatenated form tg_rank_scores avoids: fc2(relu(fc1([xp | yp]))), float64 from
              the float32 inputs, and the per-pair magnitude A that the derived tolerance scales with
score_bound   the derived tolerance per pair
numpy_ranks   the rank definition
make_case     constructed (not sampled) inputs of one score case: every hit column and every class occurs"""
import numpy as np

HIT = {'none': 0, 'vec': 1, 'bin': 2, 'count': 3}   # TG_HIT_*


def numpy_ranks(s, ids, dst, mask=None):
    s0 = s[:, :1]
    left_in = (ids[:, 1:] != dst[:, None]) & (ids[:, 1:] != 0)
    if mask is not None:
        left_in &= mask
    g = ((s[:, 1:] > s0) & left_in).sum(1)
    e = ((s[:, 1:] == s0) & left_in).sum(1)
    return g, e, left_in.sum(1), 1.0 + g.astype(np.float64) + 0.5 * e.astype(np.float64)


def pair_hits(nbr_src, nbr_cand, src, cand_ids):
    """src hits [B, 1 + C, K] = (nbr_cand[i, j, :] == src[i]), dst hits [B, 1 + C, K] = (nbr_src[i, :] == cand_ids[i, j])"""
    sh = (nbr_cand == src[:, None, None]).astype(np.float64)
    dh = (nbr_src[:, None, :] == cand_ids[:, :, None]).astype(np.float64)
    return sh, dh


def score_ref(h_src, h_cand, nbr_src, nbr_cand, src, cand_ids, w1, b1, w2, b2, hit_type, hit_emb, *, omit=()):
    """-> (scores [B, 1 + C], A [B, 1 + C]), float64.  src hits go with x, dst hits with y; 'vec' appends the hits,
    'bin' / 'count' add hit_emb[max / sum of the hits].  A = sum_n |w2_n| (sum_k |w1_nk| |z_k| + |b1_n|) + |b2| with
    |z| = |x| + |e| for 'bin' / 'count' (the kernel multiplies the embedding rows separately).
    omit: 'T_s' / 'T_d' leave the hit embedding of that side out ('bin' / 'count'; the sensitivity condition of
    tests/test_rank_ref_host.py) - every other term is taken out by zeroing its weights."""
    f8 = lambda a: np.asarray(a, dtype=np.float64)
    h_src, h_cand, w1, b1, w2, b2 = (f8(a) for a in (h_src, h_cand, w1, b1, w2, b2))
    B, C1, d = h_cand.shape
    x = np.broadcast_to(h_src[:, None, :], (B, C1, d))
    y = h_cand
    ax, ay = np.abs(x), np.abs(y)
    if hit_type != 'none':
        sh, dh = pair_hits(nbr_src, nbr_cand, src, cand_ids)
    if hit_type == 'vec':
        xp, yp = np.concatenate([x, sh], 2), np.concatenate([y, dh], 2)
        ax, ay = np.abs(xp), np.abs(yp)
    elif hit_type in ('bin', 'count'):
        emb = f8(hit_emb)
        red = (lambda t: t.max(2).astype(np.int64)) if hit_type == 'bin' else (lambda t: t.sum(2).astype(np.int64))
        es = emb[red(sh)] * (0.0 if 'T_s' in omit else 1.0)
        ed = emb[red(dh)] * (0.0 if 'T_d' in omit else 1.0)
        xp, yp = x + es, y + ed
        ax, ay = ax + np.abs(es), ay + np.abs(ed)
    else:
        xp, yp = x, y
    z = np.concatenate([xp, yp], 2)                      # [B, 1 + C, 2W]
    assert z.shape[2] == w1.shape[1], (z.shape, w1.shape)
    hid = np.maximum(z @ w1.T + b1, 0.0)
    scores = hid @ w2.reshape(-1) + b2.reshape(-1)[0]
    az = np.concatenate([ax, ay], 2)
    A = (az @ np.abs(w1).T + np.abs(b1)) @ np.abs(w2.reshape(-1)) + np.abs(b2.reshape(-1)[0])
    return scores, A


def score_bound(A, d, W):
    """|got - ref64| <= (2W + d + 8) 2^-24 A: the first-order worst case of the two float32 dot products (2W terms, then
    d terms) in any summation order, the few additions of the epilogue included; ReLU is 1-Lipschitz"""
    return (2 * W + d + 8) * 2.0 ** -24 * A


# (d, K, B, C, hit): each the smallest shape that reaches its path of k_rank_tile / k_head_half (csrc/tg_rank.hip, tg_rank_head.h)
SCORE_CASES = [
    (8, 5, 3, 1, 'bin'),       # the smallest: one tile, one k tile, `min(n, d - 1)` clamps 120 of the 128 weight rows
    (8, 6, 1, 0, 'vec'),       # P = 1: `min(m0 + tid, P - 1)` repeats the one pair in the 31 spare rows
    (30, 2, 4, 7, 'vec'),      # KX = 34: dst hits end k tile 0, src hits open k tile 1 (hit_operand: `k < K`, `k < 2 * K`); P = 32 exactly
    (32, 16, 3, 10, 'vec'),    # KX = 64, W = 48: the `k < W` weight-index switch (pair_weight) falls inside k tile 1; P = 33
    (33, 5, 31, 0, 'count'),   # wave 1 holds one column (`n < d` under `live`); C = 0; P = 31
    (96, 4, 5, 6, 'bin'),      # wave 3 is dead: `live` false for a whole wavefront
    (128, 4, 33, 1, 'none'),   # one full column pass; the source half (k_head_half) spans two tiles (B > 32); all id arrays NULL
    (129, 3, 3, 40, 'count'),  # the second `nc` pass holds one column; an event's 41 pairs straddle tiles (`p / C1`)
    (172, 10, 7, 5, 'vec'),    # KX = 192, W = 182: two column passes with hit operand columns
    (172, 10, 7, 5, 'count'),  # two column passes with class tables; n_hit_rows = K + 3 > K + 1 (EXTRA_HIT_ROWS)
]
EXTRA_HIT_ROWS = {(172, 10, 7, 5, 'count'): 2}   # rows of hit_emb beyond the K + 1 classes, per case
CASE_IDS = ['d{}-K{}-B{}-C{}-{}'.format(*c) for c in SCORE_CASES]


def make_case(d, K, B, C, hit, seed=0, extra_hit_rows=0):
    """Inputs of tg_rank_scores as float32 / int64 numpy arrays.  Neighbour ids are constructed: the last pair has all K
    hits on either side ('count': the last embedding row), pair 0 none (P >= 2), in between the src-hit count of pair p is
    p mod (K + 1) on random columns; on the dst side the slots of a source name candidates of its event so that
    every class 0 .. K occurs where B and C leave room (all 'count' cases), else one of them or nobody at random.
    Non-hitting slots hold another event's source id / another event's candidate id: a wrong event index hits.
    fc1's hit columns and hit_emb have scale 0.5 and more, so that a hit moves a score far above the tolerance."""
    rs = np.random.RandomState(1000 * d + 10 * K + B + C + seed)
    C1, W = C + 1, d + (K if hit == 'vec' else 0)
    P = B * C1
    f4 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    c = dict(d=d, K=K, B=B, C=C, hit=hit, W=W, P=P)
    c['h_src'] = f4(rs.standard_normal((B, d)))
    c['h_cand'] = f4(rs.standard_normal((B, C1, d)))
    w1 = rs.standard_normal((d, 2 * W)) / np.sqrt(2 * W)
    if hit == 'vec':
        w1[:, d:W] = rs.standard_normal((d, K)) * 0.75
        w1[:, W + d:] = rs.standard_normal((d, K)) * 0.75
    c['w1'], c['b1'] = f4(w1), f4(rs.standard_normal(d) * 0.5)
    c['w2'], c['b2'] = f4(rs.standard_normal((1, d)) / np.sqrt(d)), f4([0.25])
    c['n_hit_rows'] = {'bin': 2, 'count': K + 1 + extra_hit_rows}.get(hit, 0)
    c['hit_emb'] = f4(rs.standard_normal((c['n_hit_rows'], d)) * 0.75) if c['n_hit_rows'] else None
    src = 1000 + np.arange(B, dtype=np.int64)
    cand = 2000 + np.arange(P, dtype=np.int64).reshape(B, C1)
    nobody_s = src[(np.arange(B) + 1) % B] if B > 1 else np.full(B, 7, dtype=np.int64)       # another event's source
    nobody_d = cand[(np.arange(B) + 1) % B, 0] if B > 1 else np.full(B, 9, dtype=np.int64)   # another event's candidate
    nbr_cand = np.broadcast_to(nobody_s[:, None, None], (B, C1, K)).copy()
    nbr_src = np.broadcast_to(nobody_d[:, None], (B, K)).copy()
    for p in range(P):
        i, j = divmod(p, C1)
        n = K if p == P - 1 else (0 if p == 0 and P >= 2 else p % (K + 1))
        nbr_cand[i, j, rs.permutation(K)[:n]] = src[i]
    # dst side: the K slots of source i name candidates of event i.  The last event gives all K to its last candidate,
    # pair 0 gets none; the classes 1 .. K - 1 are dealt first, largest first, each to a candidate of its own in the
    # first event that has the slots and a candidate left; the remaining events draw at random
    todo = list(range(K - 1, 0, -1))
    for i in range(B):
        if i == B - 1:
            nbr_src[i, :] = cand[i, C1 - 1]
            continue
        free = [j for j in range(C1) if not (i == 0 and j == 0 and P >= 2)]
        k = 0
        dealt = False
        for n in list(todo):
            if free and k + n <= K:
                nbr_src[i, k:k + n] = cand[i, free.pop()]
                k += n
                todo.remove(n)
                dealt = True
        if dealt or not free:
            continue
        for k in range(K):
            j = rs.randint(-1, C1)           # -1: nobody
            if j >= 0 and j in free:
                nbr_src[i, k] = cand[i, j]
    c.update(src=src, cand_ids=cand, nbr_src=nbr_src, nbr_cand=nbr_cand)
    if hit == 'none':
        c.update(src=None, cand_ids=None, nbr_src=None, nbr_cand=None)
    return c


REF_ARGS = ('h_src', 'h_cand', 'nbr_src', 'nbr_cand', 'src', 'cand_ids', 'w1', 'b1', 'w2', 'b2', 'hit', 'hit_emb')
_REF = {}


def case_ref(key):
    """(case, float64 scores, bound per pair) of SCORE_CASES entry `key`, computed once and left unchanged"""
    if key not in _REF:
        c = make_case(*key, extra_hit_rows=EXTRA_HIT_ROWS.get(key, 0))
        s, A = score_ref(*[c[k] for k in REF_ARGS])
        for a in (s, A):
            a.setflags(write=False)
        _REF[key] = (c, s, score_bound(A, c['d'], c['W']))
    return _REF[key]


# ---- rank statistics: synthetic score matrices ----------------------------------------------------------------------------
# (B, C): 0, 1, 2 and 3 passes of k_rank_event's 64-lane `j0` loop and both sides of its boundary; 1, 2, 3 and 5 passes of
# k_rank_fold's `i += 64` loop; B not a multiple of the 4 events of a block
STATS_SHAPES = [(1, 0), (1, 1), (3, 63), (4, 64), (5, 65), (2, 129), (64, 5), (65, 5), (130, 3), (257, 70)]


def make_stats_case(B, C, seed=0):
    """scores from {-1, -0.5, 0, 0.5, 1} (ties are common), ids [B, 1 + C] with column 0 = dst, about 10 % of the
    candidates equal to dst[i] and 10 % to the padding id 0, one event (B >= 3: event B // 2) with everything left out,
    a random mask of 70 % ones"""
    rs = np.random.RandomState(77 * B + C + seed)
    s = rs.choice(np.array([-1, -0.5, 0, 0.5, 1], dtype=np.float32), (B, 1 + C))
    dst = rs.randint(1, 500, B).astype(np.int64)
    cand = rs.randint(500, 1000, (B, C)).astype(np.int64)
    u = rs.random_sample((B, C))
    cand = np.where(u < 0.1, dst[:, None], np.where(u < 0.2, 0, cand))
    if B >= 3:
        cand[B // 2] = np.where(np.arange(C) % 2 == 0, dst[B // 2], 0)
    ids = np.concatenate([dst[:, None], cand], 1)
    mask = rs.random_sample((B, C)) < 0.7
    return np.ascontiguousarray(s), ids, dst, mask
