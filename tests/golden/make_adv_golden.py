#!/usr/bin/env python3
"""Writes tests/golden/adv_neg.npz: the candidate sets of the reference's AdversarialEdgeSampler
(tiger/data/adversarial.py) on a small stream, for tests/test_adv_neg_host.py and tests/test_hip_adv_neg.py.

    python tests/golden/make_adv_golden.py --reference /path/to/www2023tiger

Needs the reference checkout (yzhang1918/www2023tiger @ v1.0.1); the tests read only the .npz.  For every query of
`pre_sample_neg_dsts` (chunks of bs = 200 and 37 test events) the script records the set the reference draws from -
hist_edge_dict[src] - current_edge_dict[src] (- train_edge_dict[src] for `ind`), built with the reference's own
get_edges_within and train_edge_dict - sorted and flattened with offsets, and full_dst_distinct.

The stream: 1500 events over 150 integer time steps (about ten events per timestamp), users 1..25 and items 26..60
with some user -> user events and two self-loops, repeated pairs, and test sources without any history (ids 61..64).
The script checks that pairs recur exactly at a chunk's t0, at its t1 and at ts_hist_end.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def make_stream(seed=11):
    rs = np.random.RandomState(seed)
    E = 1500
    ts = np.floor(np.sort(rs.uniform(0, 150, E)))
    src = rs.randint(1, 26, E)
    dst = rs.randint(26, 61, E)
    u2u = rs.uniform(size=E) < 0.08
    dst[u2u] = rs.randint(1, 26, u2u.sum())
    src[[100, 700]] = dst[[100, 700]] = 7  # self-loops
    n_test = 225
    fresh = E - n_test + rs.choice(n_test, 12, replace=False)
    src[fresh] = rs.randint(61, 65, len(fresh))  # sources first seen in the test part
    return src.astype(np.int64), dst.astype(np.int64), ts.astype(np.float64), n_test


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference checkout')
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from tiger.data.adversarial import AdversarialEdgeSampler

    src, dst, ts, n_test = make_stream()
    out = dict(src=src, dst=dst, ts=ts, n_test=np.int64(n_test))
    hits = dict(t0=0, t1=0, hist_end=0)
    for mode in ('hist', 'ind'):
        ref = AdversarialEdgeSampler(src, dst, ts, src[-n_test:], ts[-n_test:], mode, seed=0)
        out['full_dst_distinct'] = ref.full_dst_distinct.astype(np.int64)
        out['ts_hist_end'] = np.float64(ref.ts_hist_end)
        for bs in (200, 37):
            vals, off = [], [0]
            for c in range(0, n_test, bs):
                srcs = ref.test_srcs[c:c + bs]
                t = ref.test_ts[c:c + bs]
                t0, t1 = t[0], t[-1]
                hist = ref.get_edges_within(ref.ts_init, t0, srcs)
                cur = ref.get_edges_within(t0, t1, srcs)
                for s in srcs:
                    cand = hist[s] - cur[s]
                    if mode == 'ind':
                        cand = cand - ref.train_edge_dict[s]
                    vals.extend(sorted(int(d) for d in cand))
                    off.append(len(vals))
                    pairs = hist[s]
                    at = lambda tt: sum(1 for d in pairs if np.any((src == s) & (dst == d) & (ts == tt)))
                    hits['t0'] += at(t0)
                    hits['t1'] += at(t1)
                    hits['hist_end'] += at(ref.ts_hist_end)
            out[f'{mode}_{bs}_vals'] = np.array(vals, dtype=np.int64)
            out[f'{mode}_{bs}_off'] = np.array(off, dtype=np.int64)
    assert all(v > 0 for v in hits.values()), hits
    sizes = np.diff(out['hist_200_off'])
    assert (sizes == 0).any() and (sizes >= 5).any()
    np.savez_compressed(os.path.join(HERE, 'adv_neg.npz'), **out)
    print('adv_neg.npz:', {k: v.shape for k, v in out.items()}, 'recurrences', hits)


if __name__ == '__main__':
    main()
