"""Historical / inductive negative sampling on the host (no GPU): the library's host twins of the pair index and the
sampler (csrc/tg_adv.hip) against the reference's candidate sets (tests/golden/adv_neg.npz, written by
make_adv_golden.py from tiger/data/adversarial.py), numpy restatements of the index and of the documented draw, and
the behaviour of www2023tiger_amd.data.adversarial.AdversarialEdgeSampler."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'adv_neg.npz')
M32 = np.uint64(0xFFFFFFFF)


def golden():
    return np.load(GOLDEN)


def sampler(src, dst, ts, n_test, mode, seed=5, device='cpu', **kw):
    from www2023tiger_amd.data.adversarial import AdversarialEdgeSampler
    return AdversarialEdgeSampler(src, dst, ts, src[-n_test:], ts[-n_test:], mode, seed=seed, device=device, **kw)


def chunk_windows(test_ts, bs):
    n = len(test_ts)
    first = (np.arange(n) // bs) * bs
    last = np.minimum(first + bs, n) - 1
    return test_ts[first].astype(np.float64), test_ts[last].astype(np.float64)


def mix32(x):
    x = x.astype(np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def adv_hash(seed, counter, q, s):
    """tiger_hip.h: tg_adv_hash, restated in numpy (q: array of query indices)"""
    k = (int(seed) ^ (int(counter) * 0x9E3779B97F4A7C15)) & (2 ** 64 - 1)
    q = np.asarray(q, dtype=np.uint64)
    h = mix32((q & M32) ^ np.uint64(k & 0xFFFFFFFF))
    h = mix32(h + (((q >> np.uint64(32)) * np.uint64(0x9e3779b9)) & M32) + np.uint64(k >> 32))
    return mix32(h ^ np.uint64((s * 0x85ebca6b) & 0xFFFFFFFF))


def mulhi32(h, c):
    return (h.astype(np.uint64) * np.asarray(c, dtype=np.uint64)) >> np.uint64(32)


def index_numpy(indptr, ts, nbr, eid):
    """(next_ts, first_ts) by a lexsort of the out-entries on (owner, neighbour, position)"""
    P = len(ts)
    owner = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    out = (eid.view(np.uint32) >> np.uint32(31)) == 0
    nxt = np.full(P, -np.inf)
    fst = np.full(P, -np.inf)
    pos = np.nonzero(out)[0]
    o = pos[np.lexsort((pos, nbr[pos], owner[pos]))]
    same_next = np.zeros(len(o), dtype=bool)
    same_next[:-1] = (owner[o[1:]] == owner[o[:-1]]) & (nbr[o[1:]] == nbr[o[:-1]])
    nxt[o] = np.where(same_next, np.concatenate([ts[o[1:]], [np.inf]]), np.inf)
    head = np.ones(len(o), dtype=bool)
    head[1:] = ~same_next[:-1]
    group_start = np.maximum.accumulate(np.where(head, np.arange(len(o)), 0))
    fst[o] = ts[o[group_start]]
    return nxt, fst


def expected_draws(a, srcs, t0, t1, mode, seed, counter):
    """the documented draw over the host T-CSR and index (numpy): (negatives, counts, candidate lists)"""
    indptr, ts, nbr, _ = a.graph._host_tcsr()
    nxt, fst = a._index()
    dd = np.asarray(a.full_dst_distinct, dtype=np.int64)
    negs, counts, cands = [], [], []
    h_pick = adv_hash(seed, counter, np.arange(len(srcs)), 7)
    h_fb = adv_hash(seed, counter, np.arange(len(srcs)), 8)
    for q, s in enumerate(srcs):
        if 0 <= s < len(indptr) - 1:
            lo = indptr[s]
            end = lo + np.searchsorted(ts[lo:indptr[s + 1]], t0[q], side='left')
            e = np.arange(lo, end)
        else:
            e = np.arange(0)
        ok = nxt[e] > t1[q]
        if mode == 'ind':
            ok &= fst[e] > a.ts_hist_end
        c = e[ok]
        cands.append(nbr[c].astype(np.int64))
        counts.append(len(c))
        negs.append(nbr[c[int(mulhi32(h_pick[q:q + 1], len(c))[0])]] if len(c) else dd[int(mulhi32(h_fb[q:q + 1], len(dd))[0])])
    return np.array(negs, dtype=np.int64), np.array(counts), cands


@pytest.mark.parametrize('mode', ['hist', 'ind'])
@pytest.mark.parametrize('bs', [200, 37])
def test_host_sampler_against_the_reference_sets(mode, bs):
    """per query: the count equals the size of the reference's set, the candidates (T-CSR order) are that set, every
    negative lies in it (or in full_dst_distinct when it is empty), and each draw is the documented hash's"""
    z = golden()
    n = int(z['n_test'])
    a = sampler(z['src'], z['dst'], z['ts'], n, mode, seed=5)
    np.testing.assert_array_equal(a.full_dst_distinct, z['full_dst_distinct'])
    assert a.ts_hist_end == z['ts_hist_end']
    vals, off = z[f'{mode}_{bs}_vals'], z[f'{mode}_{bs}_off']
    srcs = a.test_srcs
    t0, t1 = chunk_windows(a.test_ts, bs)
    negs, cnt = a._launch({'hist': 0, 'ind': 1}[mode], np.ascontiguousarray(srcs, dtype=np.int64), t0, t1, 0,
                          out_count=True)
    np.testing.assert_array_equal(cnt, np.diff(off))
    exp_negs, exp_cnt, cands = expected_draws(a, srcs, t0, t1, mode, 5, 0)
    np.testing.assert_array_equal(exp_cnt, np.diff(off))
    np.testing.assert_array_equal(negs, exp_negs)
    for q in range(n):
        ref_set = vals[off[q]:off[q + 1]]
        np.testing.assert_array_equal(np.sort(cands[q]), ref_set)
        if len(ref_set):
            assert negs[q] in ref_set
        else:
            assert negs[q] in z['full_dst_distinct']
    np.testing.assert_array_equal(a.pre_sample_neg_dsts(n, bs=bs), negs)  # one call, counter 0


@pytest.mark.parametrize('mode', ['hist', 'ind'])
def test_set_helpers_restate_the_reference_sets(mode):
    """get_edges_within / train_edge_dict (the reference's set-based helpers, kept for API parity) give the same sets"""
    z = golden()
    n = int(z['n_test'])
    a = sampler(z['src'], z['dst'], z['ts'], n, mode)
    vals, off = z[f'{mode}_37_vals'], z[f'{mode}_37_off']
    for c in range(0, n, 37):
        srcs, t = a.test_srcs[c:c + 37], a.test_ts[c:c + 37]
        hist, cur = a.get_edges_within(a.ts_init, t[0], srcs), a.get_edges_within(t[0], t[-1], srcs)
        for i, s in enumerate(srcs):
            cand = hist[s] - cur[s] - (a.train_edge_dict[s] if mode == 'ind' else set())
            np.testing.assert_array_equal(np.array(sorted(cand), dtype=np.int64), vals[off[c + i]:off[c + i + 1]])


def _streams():
    import bench
    z = golden()
    st = bench.make_stream(300, 80, 6000, 2000.0, seed=3, with_efeats=False)
    return [(z['src'], z['dst'], z['ts']), (st['src'], st['dst'], st['ts'])]


def test_host_index_equals_a_lexsort_restatement():
    for src, dst, ts in _streams():
        a = sampler(src, dst, ts, 100, 'hist')
        nxt, fst = a._index()
        e_nxt, e_fst = index_numpy(*a.graph._host_tcsr())
        np.testing.assert_array_equal(nxt, e_nxt)
        np.testing.assert_array_equal(fst, e_fst)
        eid = a.graph._host_tcsr()[3].view(np.uint32)
        assert np.all(np.isneginf(nxt[eid >> 31 == 1])) and np.all(nxt[eid >> 31 == 0] > -np.inf)


def test_sampler_api_behaviour():
    from www2023tiger_amd.data.adversarial import AdversarialEdgeSampler
    z = golden()
    n = int(z['n_test'])
    src, dst, ts = z['src'], z['dst'], z['ts']
    a = sampler(src, dst, ts, n, 'hist', seed=9)
    x = a.pre_sample_neg_dsts(n)
    y = a.pre_sample_neg_dsts(n)
    assert x.dtype == np.int64 and len(x) == n
    np.testing.assert_array_equal(x, y)
    a.reset_random_state()
    s0, n0 = a.sample(a.test_srcs[:150], a.test_ts[0], a.test_ts[149])
    s1, n1 = a.sample(a.test_srcs[:150], a.test_ts[0], a.test_ts[149])
    np.testing.assert_array_equal(s0, a.test_srcs[:150])
    assert isinstance(n0, np.ndarray) and not np.array_equal(n0, n1)  # every call advances the counter
    a.reset_random_state()
    np.testing.assert_array_equal(a.sample(a.test_srcs[:150], a.test_ts[0], a.test_ts[149])[1], n0)
    with pytest.raises(ValueError, match='Undefined Negative Edge Sampling Strategy!'):
        AdversarialEdgeSampler(src, dst, ts, src[-n:], ts[-n:], 'rnd', device='cpu')
    a.neg_type = 'bogus'
    with pytest.raises(ValueError, match='Undefined Negative Edge Sampling Strategy!'):
        a.sample(src[:3], 1.0, 2.0)
    a.neg_type = 'hist'
    with pytest.raises(ValueError, match='t0'):
        a.sample(src[:3], 5.0, 4.0)
    bad = ts.copy()
    bad[[10, 20]] = bad[[20, 10]] + np.array([0.0, 1.0])
    with pytest.raises(ValueError, match='sorted'):
        AdversarialEdgeSampler(src, dst, bad, src[-n:], bad[-n:], 'hist', device='cpu')
    # seed None: a fresh stream at every reset (RandomState(None)), the same sets
    b = sampler(src, dst, ts, n, 'hist', seed=None)
    assert not np.array_equal(b.pre_sample_neg_dsts(n), b.pre_sample_neg_dsts(n))
    # attributes of the reference's constructor
    for k in ('full_srcs_distinct', 'full_dst_distinct', 'full_ts_distinct', 'ts_init', 'ts_end', 'ts_hist_end',
              'train_edge_dict', 'test_srcs', 'test_ts', 'seed', 'neg_type'):
        assert hasattr(a, k), k
    assert a.ts_init == ts.min() and a.ts_end == ts.max() and a.ts_hist_end == ts[-n - 1]


def test_host_entry_points_refuse_bad_arguments():
    from www2023tiger_amd import _lib
    z = golden()
    a = sampler(z['src'], z['dst'], z['ts'], int(z['n_test']), 'hist')
    nxt, fst = a._index()
    ix = _lib.TgAdvIndex(_lib.ptr(nxt), _lib.ptr(fst))
    g = a._tcsr_h
    srcs = np.array([3, 4], dtype=np.int64)
    dd = np.array([30, 31], dtype=np.int64)
    out = np.empty(2, dtype=np.int64)

    def call(t0, t1, mode=0, n_dd=2):
        return _lib.lib.tg_adv_neg_sample_host(C.byref(g), C.byref(ix), 2, _lib.ptr(srcs), _lib.ptr(t0), _lib.ptr(t1), mode,
                                               0.0, _lib.ptr(dd), n_dd, 1, 0, _lib.ptr(out), None)
    good = np.array([50.0, 60.0]), np.array([55.0, 60.0])
    assert call(*good) == _lib.TG_OK
    assert call(np.array([50.0, 61.0]), np.array([55.0, 60.0])) == _lib.TG_EINVAL  # t0 > t1
    assert call(*good, mode=2) == _lib.TG_EINVAL
    assert call(*good, n_dd=0) == _lib.TG_EINVAL
    # ids outside [0, num_node) have no candidates: the fallback
    srcs[:] = [-1, 10 ** 6]
    cnt = np.empty(2, dtype=np.int64)
    assert _lib.lib.tg_adv_neg_sample_host(C.byref(g), C.byref(ix), 2, _lib.ptr(srcs), _lib.ptr(good[0]), _lib.ptr(good[1]),
                                           0, 0.0, _lib.ptr(dd), 2, 1, 0, _lib.ptr(out), _lib.ptr(cnt)) == _lib.TG_OK
    assert list(cnt) == [0, 0] and set(out) <= {30, 31}


def test_draws_are_uniform_over_a_five_candidate_set():
    """fixed seed: 20000 queries of one source with exactly five historical destinations; chi-square, 4 degrees of
    freedom, below its 0.1 % quantile (18.47)"""
    src = np.array([1, 1, 1, 1, 1, 2, 1, 2], dtype=np.int64)
    dst = np.array([10, 11, 12, 13, 14, 10, 11, 12], dtype=np.int64)
    ts = np.array([1.0, 2.0, 3.0, 3.0, 4.0, 5.0, 5.0, 6.0])
    a = sampler(src, dst, ts, 2, 'hist', seed=1234)
    n = 20000
    negs, cnt = a._launch(0, np.ones(n, dtype=np.int64), np.full(n, 10.0), np.full(n, 10.0), 0, out_count=True)
    assert np.all(cnt == 5)
    f = np.bincount(negs - 10, minlength=5)
    assert f.sum() == n and len(f) == 5
    chi2 = float(((f - n / 5) ** 2 / (n / 5)).sum())
    assert chi2 < 18.47, (f, chi2)
    # the pair 1 -> 11 recurs at 5.0: a window [4.5, 5.0] leaves four candidates, [5.0, 5.0] (t0 itself) too
    for t0 in (4.5, 5.0):
        _, c = a._launch(0, np.ones(1, dtype=np.int64), np.array([t0]), np.array([5.0]), 0, out_count=True)
        assert c[0] == 4


def test_adv_index_struct_layout_matches_the_header(tmp_path):
    from www2023tiger_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tiger_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %zu\\n", sizeof(tg_adv_index), offsetof(tg_adv_index, next_ts), '
             'offsetof(tg_adv_index, first_ts));', '  printf("%d %d\\n", TG_ADV_HIST, TG_ADV_IND);', '  return 0;', '}']
    src = tmp_path / 'adv_layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'adv_layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    l1, l2 = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')[:2]
    assert [int(v) for v in l1.split()] == [C.sizeof(_lib.TgAdvIndex), _lib.TgAdvIndex.next_ts.offset,
                                            _lib.TgAdvIndex.first_ts.offset]
    assert [int(v) for v in l2.split()] == [_lib.TG_ADV_HIST, _lib.TG_ADV_IND]
