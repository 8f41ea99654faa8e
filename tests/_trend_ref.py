"""Reference, sizes and cases of the trending-candidate tests (tests/test_trend_host.py, tests/test_hip_trend.py).

The reference is written from the contracts of tg_trending and tg_fill_candidates (include/tiger_hip.h) and shares nothing
with the library: per-node time rows from one np.lexsort (_walk_ref.WalkRef), np.searchsorted(side='left') for both bounds of
the window and for the seen prefix, sorted(key=(-c, id)) for the order and a plain Python loop for the fill.  Everything is
integer work: every comparison in the tests is exact."""
import numpy as np

import _cap_ref
import _walk_ref as W

TREND_MAX = 2048       # `#define TG_TREND_MAX 2048`
TILE = 2048            # tg_trend.hip: `constexpr int TR_TILE = 2048;`
# tg_trend.hip: tg_trending: `dim3(flat_grid(n_pad, TR_GROUPS))`, TR_GROUPS = 256 / 16 nodes per workgroup and pass
NODES_PER_WORKGROUP = _cap_ref.PER_16_LANES
CAP_KEYS = _cap_ref.FLAT_BLOCKS * NODES_PER_WORKGROUP      # 65 536 nodes: the last size without a second pass
N_KEYS_PAST = _cap_ref.past(CAP_KEYS, 5)
# tg_trend.hip: tg_fill_candidates: `dim3(flat_grid(B, 1))` - one workgroup per query
CAP_FILL = _cap_ref.FLAT_BLOCKS
B_FILL_PAST = _cap_ref.past(CAP_FILL, 5)

MS = (0, 1, 15, 16, 17, 255, 256, 257, 2047, 2048, 2049, 4097)
TS = (1, 16, 64, 2048)
FILL_CS = (1, 16, 64, 512, 2048)
FILL_TS = (1, 255, 256, 257, 2048)
WIDE_N = 5000          # the small graph's events over 5 000 node ids: `among` lists of up to 4 097 distinct ids
NAMES = W.NAMES
FILL_NAMES = ('ids', 'counts', 'n_valid', 'n_filled')


# ---- the reference ---------------------------------------------------------------------------------------------------------
def count(ref, v, t_lo, t_hi):
    """entries of v with t_lo <= time < t_hi"""
    if not 0 <= v < ref.N:
        return 0
    row = ref.t[v]
    return int(np.searchsorted(row, t_hi, side='left')) - int(np.searchsorted(row, t_lo, side='left'))


def trending(ref, t, T, window=None, among=None):
    """-> dict(ids int64 [T], counts int32 [T], n_valid int32 [1], n_distinct int32 [1])"""
    t_hi = float(t)
    t_lo = -np.inf if window is None else t_hi - float(window)
    nodes = range(1, ref.N) if among is None else [int(v) for v in among]
    c = [(v, count(ref, v, t_lo, t_hi)) for v in nodes if v != 0]
    best = sorted([vc for vc in c if vc[1] > 0], key=lambda vc: (-vc[1], vc[0]))
    k = min(T, len(best))
    ids, counts = np.zeros(T, np.int64), np.zeros(T, np.int32)
    ids[:k] = [v for v, _ in best[:k]]
    counts[:k] = [n for _, n in best[:k]]
    return dict(ids=ids, counts=counts, n_valid=np.array([k], np.int32), n_distinct=np.array([len(best)], np.int32))


def fill(ref, src, ts, cand, fill_ids, n_fill, exclude_seen=False, keep_self=False):
    """cand: dict(ids [B, C], counts [B, C], n_valid [B]) of arrays, left as they are -> dict(ids, counts, n_valid, n_filled)"""
    ids, counts, n_valid = (np.array(cand[k]) for k in ('ids', 'counts', 'n_valid'))
    B, C = ids.shape
    n_filled = np.zeros(B, np.int32)
    take = [int(v) for v in fill_ids[:max(0, min(int(n_fill), len(fill_ids)))]]
    for i in range(B):
        nv = int(n_valid[i])
        if nv >= C:
            continue
        out = set(ids[i, :nv].tolist())
        if not keep_self:
            out.add(int(src[i]))
        if exclude_seen:
            out |= set(ref.prefix(int(src[i]), ts[i]).tolist())
        at = nv
        for v in take:
            if at == C:
                break
            if v == 0 or v in out:
                continue
            out.add(v)
            ids[i, at], counts[i, at] = v, 0
            at += 1
        n_filled[i], n_valid[i] = at - nv, at
    return dict(ids=ids, counts=counts, n_valid=n_valid, n_filled=n_filled)


def assert_same(got, want, what='', names=NAMES):
    for name in names:
        g = got[name]
        g = g.cpu().numpy() if hasattr(g, 'cpu') else np.asarray(g)
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        np.testing.assert_array_equal(g, want[name], err_msg=f'{what}: {name}')


# ---- the library -----------------------------------------------------------------------------------------------------------
def tensor(a, device, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype)).to(device)


def library_trending(graph, t, T, device, window=None, among=None):
    from www2023tiger_amd import hip_ops
    return hip_ops.trending(graph, t, T, window=window, among=None if among is None else tensor(among, device, np.int64))


def library_fill(graph, src, ts, cand, fill_ids, n_fill, device, **flags):
    from www2023tiger_amd import hip_ops
    c = dict(ids=tensor(cand['ids'], device, np.int64), counts=tensor(cand['counts'], device, np.int32),
             n_valid=tensor(cand['n_valid'], device, np.int32))
    keep = {k: v.clone() for k, v in c.items()}
    trend = dict(ids=tensor(fill_ids, device, np.int64), n_valid=tensor(np.array([n_fill]), device, np.int32))
    out = hip_ops.fill_candidates(graph, tensor(src, device, np.int64), tensor(ts, device, np.float64), c, trend, **flags)
    import torch
    assert all(torch.equal(c[k], keep[k]) for k in c), "the caller's tensors were written"
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------
_WIDE = {}


def wide_case():
    """_cap_ref.small_graph() over WIDE_N node ids (ids from 400 on have no entries) -> (N, events, reference)"""
    if not _WIDE:
        _, src, dst, ts, eids = _cap_ref.small_graph()
        _WIDE['case'] = (WIDE_N, (src, dst, ts, eids), W.WalkRef(WIDE_N, src, dst, ts))
    return _WIDE['case']


def among_list(M, seed):
    """M distinct ids of the wide graph in random order; node 0 and the hub 9 are in every list that has room for them"""
    rs = np.random.RandomState(seed)
    ids = rs.permutation(WIDE_N)[:M].astype(np.int64)
    for pos, v in ((M // 2, 0), (M - 1, 9)):
        if M >= 15 and v not in ids:
            ids[pos] = v
    assert len(set(ids.tolist())) == M
    return ids


def windows():
    """(name, t, window) over the small graph, whose times are whole numbers with duplicates"""
    _, (_, _, ts, _), _ = wide_case()
    t_max = float(ts.max())
    on = np.unique(ts)
    lo, hi = float(on[len(on) // 3]), float(on[2 * len(on) // 3])       # both bounds ON event times
    return (('all', t_max + 1.0, None), ('on-events', hi, hi - lo), ('empty', hi, 1e-6), ('before-everything', -1.0, None),
            ('before-everything-window', float(ts.min()), 50.0), ('wider-than-history', t_max + 10.0, 1e9),
            ('half', t_max / 2, None), ('recent', t_max + 1.0, 40.0))


TIE_ITEMS, TIE_FIRST, TIE_HEAVY = 3000, 100, (1500, 2900, 120)


def tie_case():
    """Items 100 .. 3099 with two entries each but three with five; `among` lists the items so that the smallest ids - the
    ones ascending id picks from the tie - lie around position 2 048, the tile edge -> (N, events, among)"""
    items = np.arange(TIE_FIRST, TIE_FIRST + TIE_ITEMS, dtype=np.int64)
    dst = np.concatenate([np.repeat(items, 2), np.repeat(np.array(TIE_HEAVY, np.int64), 3)])
    src = np.full(len(dst), 1, np.int64)
    E = len(dst)
    ev = (src, dst, np.arange(1, E + 1, dtype=np.float64), np.arange(1, E + 1, dtype=np.int64))
    among = np.roll(items[::-1], -(TIE_ITEMS - TILE - 30))    # descending ids, rolled: id 129 sits at position 2 048, id 100 at 2 077
    return TIE_FIRST + TIE_ITEMS, ev, among


DEGREES = (0, 1, 16, 17, 288, 289)    # the probe rounds of prefix_end_group<16>: one up to 16, two up to 288, then three


def degree_case():
    """node 10 + k has DEGREES[k] entries at times 1 .. degree, all with node 1 -> (N, events, among)"""
    src, dst, ts = [], [], []
    for k, deg in enumerate(DEGREES):
        src.extend([10 + k] * deg), dst.extend([1] * deg), ts.extend(range(1, deg + 1))
    order = np.argsort(np.array(ts, np.float64), kind='stable')
    ev = (np.array(src, np.int64)[order], np.array(dst, np.int64)[order], np.array(ts, np.float64)[order],
          np.arange(1, len(src) + 1, dtype=np.int64))
    return 20, ev, np.arange(10, 10 + len(DEGREES), dtype=np.int64)


def fill_universe(T, seed):
    """a fill list of T slots over the wide graph: every active id first in line to collide with rows and prefixes, id 0
    inside, distinct; n_fill < T where T allows it and non-zero garbage behind it -> (fill_ids [T], n_fill)"""
    rs = np.random.RandomState(seed)
    active = rs.permutation(np.arange(0, 400, dtype=np.int64))
    rest = rs.permutation(np.arange(400, WIDE_N, dtype=np.int64))
    ids = np.concatenate([active, rest])[:T].copy()
    n_fill = T if T < 255 or T == 256 else T - 3
    ids[n_fill:] = rs.randint(1, 380, T - n_fill)    # garbage behind the list: live ids that nothing may append
    return ids, n_fill


def fill_rows(B, C, seed, sentinel=-7):
    """caller-made rows over the wide graph: n_valid cycles through 0, 1, C - 1, C and random values, the ids in front are
    distinct live ids (row 5 repeats one), the columns behind n_valid hold a sentinel -> (src, ts, cand)"""
    rs = np.random.RandomState(seed)
    _, (_, _, ts, _), _ = wide_case()
    src, t = _cap_ref.queries(400, B, float(ts.max()), seed=seed)
    src[:4] = (9, 450, 0, 17)                                  # the hub, a cold source, node 0, an ordinary one
    ids, counts = np.full((B, C), sentinel, np.int64), np.full((B, C), sentinel, np.int32)
    n_valid = np.zeros(B, np.int32)
    for i in range(B):
        nv = (0, 1, C - 1, C)[i % 4] if i % 8 < 4 else int(rs.randint(0, C + 1))
        nv = max(0, min(nv, C))
        row = rs.permutation(np.arange(1, 1500))[:nv] if nv <= 1499 else rs.permutation(np.arange(1, WIDE_N))[:nv]
        ids[i, :nv], counts[i, :nv], n_valid[i] = row, rs.randint(1, 9, nv), nv
        if i == 5 and nv >= 2:
            ids[i, 1] = ids[i, 0]
    return src, t, dict(ids=ids, counts=counts, n_valid=n_valid)


def sweep_fill_case(n):
    """_walk_ref.sweep_case(n) plus one entry of the source EXACTLY at the query's time, with the unused node 5: the source's
    prefix has n entries, X = 3 was seen long ago, Y = 4 never, and node 5 is not seen yet -> (N, events, src, ts, fill_ids)"""
    N, ev, src, ts = W.sweep_case(n)
    s, d, t, e = ev
    ev = (np.r_[s, W.SWEEP_S], np.r_[d, 5], np.r_[t, ts[0]], np.r_[e, len(e) + 1])
    fill_ids = np.array([W.SWEEP_X, 5, W.SWEEP_Y, W.SWEEP_S, 0, 10, 11, 59, W.SWEEP_U], np.int64)
    return N, ev, src, ts, fill_ids


def stride_fill_case():
    """_walk_ref.stride_case(): its 2 048 end ids as the fill list (the longest probe chains of a power-of-two-masked hash),
    queries from the source, a co-user that has seen eight of them, and a cold node -> (N, events, src, ts, fill_ids)"""
    N, ev, _, ts = W.stride_case()
    fill_ids = np.ascontiguousarray(ev[1][-2048:])
    assert len(set(fill_ids.tolist())) == 2048
    src = np.array([70000, 100, 355, 69999, 1], np.int64)
    return N, ev, src, np.full(len(src), ts[0]), fill_ids
