#!/usr/bin/env python3
"""Historical / inductive negative sampling measurements (one JSON line): at Wikipedia-, Reddit- and LastFM-shaped
synthetic streams (bench.make_stream, as tools/node_task_bench.py generates them; last 15 % of the events as the test
split, chunks of 200), the device pair-index build and the device pre-sample (tg_adv_neg_sample over every test
event in one launch) timed with HIP events after warm-up, AdversarialEdgeSampler.pre_sample_neg_dsts end to end on
the device and on the host twin, and a literal set-based Python restatement of the per-chunk sampling over its first
20 chunks, extrapolated to all chunks.  Also the sum and the maximum of the scanned prefix lengths (entries of the
query's source before t0), which with 8 (hist) or 16 (ind) bytes per entry, read twice, bound the kernel's traffic.

    python tools/adv_neg_bench.py [--shapes wiki,reddit,lastfm] [--reps R] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from collections import defaultdict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from www2023tiger_amd._lib import TgAdvIndex, check, lib, ptr  # noqa: E402
from www2023tiger_amd.data.adversarial import AdversarialEdgeSampler  # noqa: E402
from www2023tiger_amd.hip_ops import stream_ptr  # noqa: E402

SHAPES = {
    'wiki': dict(n_u=8227, n_i=1000, E=157474, T=2.68e6),
    'reddit': dict(n_u=10000, n_i=984, E=672447, T=2.68e6),
    'lastfm': dict(n_u=980, n_i=1000, E=1293103, T=1.37e8),
}
BS = 200


def timed(fn, reps, warm=2):
    """median ms of fn() between HIP events"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def wall(fn, reps=1):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def prefix_lengths(s, srcs, t0):
    """per query: the entries of its source with ts < t0 (the kernel's scan)"""
    indptr, ts, _, _ = s.graph._host_tcsr()
    owner = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    span = float(ts.max() - ts.min()) + 1.0
    key = owner * span + (ts - ts.min())  # integer timestamps: exact in float64 at these sizes
    q = srcs * span + (t0 - ts.min())
    return np.searchsorted(key, q, side='left') - indptr[srcs]


def python_restatement(full_src, full_dst, full_ts, test_src, test_ts, n_chunks, seed=0):
    """the per-chunk `hist` sampling with Python sets (what the reference computes), first n_chunks chunks"""
    rng = np.random.RandomState(seed)
    dd = np.unique(full_dst)
    t_init = full_ts[0]
    out = []
    for c in range(n_chunks):
        srcs = test_src[c * BS:(c + 1) * BS]
        t = test_ts[c * BS:(c + 1) * BS]
        want = set(srcs.tolist())

        def edges(a, b):
            lo, hi = np.searchsorted(full_ts, a, 'left'), np.searchsorted(full_ts, b, 'right')
            d = defaultdict(set)
            for s, x in zip(full_src[lo:hi], full_dst[lo:hi]):
                if s in want:
                    d[s].add(x)
            return d
        hist, cur = edges(t_init, t[0]), edges(t[0], t[-1])
        for s in srcs:
            cand = hist[s] - cur[s]
            out.append(rng.choice(list(cand)) if cand else dd[rng.randint(0, len(dd))])
    return out


def measure(name, cfg, reps):
    st = bench.make_stream(cfg['n_u'], cfg['n_i'], cfg['E'], cfg['T'], seed=0, with_efeats=False)
    src, dst, ts = st['src'], st['dst'], st['ts']
    n_test = int(round(0.15 * len(src)))
    dev = torch.device('cuda', 0)
    res = dict(shape=name, events=len(src), test_events=n_test, chunks=-(-n_test // BS))
    d = AdversarialEdgeSampler(src, dst, ts, src[-n_test:], ts[-n_test:], 'hist', seed=0, device=dev)
    d._index()
    g = d.graph.tcsr
    P = int(g.num_entry)
    nxt = torch.empty(P, dtype=torch.float64, device=dev)
    fst = torch.empty(P, dtype=torch.float64, device=dev)
    nbytes = int(lib.tg_adv_index_build_device_workspace_bytes(P, d.graph.num_node))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    res['index_build_device_ms'] = round(timed(lambda: check(lib.tg_adv_index_build_device(
        C.byref(g), ptr(nxt), ptr(fst), ptr(ws), nbytes, stream_ptr(dev)), 'build'), reps), 3)
    assert torch.equal(nxt, d._ix[0]) and torch.equal(fst, d._ix[1])
    test_ts = ts[-n_test:]
    first = (np.arange(n_test) // BS) * BS
    t0 = test_ts[first]
    t1 = test_ts[np.minimum(first + BS, n_test) - 1]
    srcs = src[-n_test:]
    q = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (srcs, t0, t1)]
    out = torch.empty(n_test, dtype=torch.int64, device=dev)
    ix = TgAdvIndex(ptr(d._ix[0]), ptr(d._ix[1]))
    for mode, m in (('hist', 0), ('ind', 1)):
        res[f'{mode}_kernel_ms'] = round(timed(lambda: check(lib.tg_adv_neg_sample(
            C.byref(g), C.byref(ix), n_test, ptr(q[0]), ptr(q[1]), ptr(q[2]), m, float(d.ts_hist_end), ptr(d._dd),
            len(d._dd), 0, 0, ptr(out), None, stream_ptr(dev)), 'sample'), reps), 3)
        s = d if mode == 'hist' else AdversarialEdgeSampler(src, dst, ts, srcs, test_ts, mode, seed=0, graph=d.graph,
                                                            device=dev)
        s.pre_sample_neg_dsts(n_test)
        res[f'{mode}_pre_sample_device_ms'] = round(wall(lambda: s.pre_sample_neg_dsts(n_test), reps), 3)
        h = AdversarialEdgeSampler(src, dst, ts, srcs, test_ts, mode, seed=0, device='cpu')
        t = time.perf_counter()
        h._index()
        res[f'{mode}_index_build_host_ms'] = round((time.perf_counter() - t) * 1e3, 3)
        res[f'{mode}_pre_sample_host_ms'] = round(wall(lambda: h.pre_sample_neg_dsts(n_test)), 3)
        assert np.array_equal(h.pre_sample_neg_dsts(n_test), s.pre_sample_neg_dsts(n_test))
    pl = prefix_lengths(d, srcs, t0)
    res['prefix_sum'] = int(pl.sum())
    res['prefix_max'] = int(pl.max())
    res['byte_bound_hist_MB'] = round(pl.sum() * 8 * 2 / 1e6, 3)
    res['byte_bound_ind_MB'] = round(pl.sum() * 16 * 2 / 1e6, 3)
    nc = min(20, res['chunks'])
    t = time.perf_counter()
    python_restatement(src, dst, ts, srcs, test_ts, nc)
    ms = (time.perf_counter() - t) * 1e3
    res['python_first_chunks'] = nc
    res['python_extrapolated_ms'] = round(ms * res['chunks'] / nc, 1)
    res['speedup_device_kernel_vs_host_twin'] = round(res['hist_pre_sample_host_ms'] / res['hist_kernel_ms'], 1)
    res['speedup_device_end_to_end_vs_python'] = round(res['python_extrapolated_ms'] / res['hist_pre_sample_device_ms'], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='wiki,reddit,lastfm')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    rows = [measure(s, SHAPES[s], a.reps) for s in a.shapes.split(',')]
    line = json.dumps(dict(tool='adv_neg_bench', device=torch.cuda.get_device_name(0), bs=BS, results=rows))
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
