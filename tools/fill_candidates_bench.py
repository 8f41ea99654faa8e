#!/usr/bin/env python3
"""Trending / back-fill measurements (one JSON line, also written to profiles/fill_candidates_v1.json), with the stream and
the method of tools/walk_candidates_bench.py: the C2-shaped synthetic stream (graph over the whole stream; no model is
involved), HIP events around `--inner` back-to-back calls on preallocated outputs after a warm-up call, `--reps` (>= 30)
samples, median / min / max per call.

  (a) trending   tg_trending, T = 256, over M = 1 000 eligible nodes (the stream's destinations, `among`) and over a
                 synthetic graph of 10^6 nodes (among = NULL: the stream's events spread over 10^6 ids); the whole history
                 and a window of a tenth of it
  (b) fill       tg_fill_candidates at B = 1 / 200 / 1 024, C = 256, T = 256, on the walk's own rows, with and without
                 exclude_seen, beside tg_walk_candidates (fan-out 10, 10, 10; levels 1 and 3) on the same queries in the
                 same run.  The rows are restored by a device copy before every fill (a filled row is full and would
                 leave at once); the copy is inside the timed region and is reported alone as `restore`.
  (c) recall     coverage_walk -> coverage over the stream's last 100 batches of 200: the share of events whose true
                 destination is among the C = 256 walk candidates, and among them after the back-fill from the T = 256
                 most active destinations before the batch's earliest event; with and without exclude_seen
Nothing is asserted and there is no threshold: nothing exists to measure against.  The stream is Zipf by construction, so
its recall gain says nothing about real data.

    python tools/fill_candidates_bench.py [--reps 30] [--out profiles/fill_candidates_v1.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bench  # noqa: E402
from walk_candidates_bench import BS, TAKE, stats, timed, walk_call  # noqa: E402
from www2023tiger_amd import hip_ops  # noqa: E402
from www2023tiger_amd._lib import check, lib, ptr  # noqa: E402
from www2023tiger_amd.data.graph import Graph  # noqa: E402

FANOUT = (10, 10, 10)
BATCHES = (1, 200, 1024)
CN = T = 256
BIG_N = 10 ** 6


def trending_call(graph, t_lo, t_hi, among, reps, inner):
    dev = torch.device(graph.device)
    n = graph.num_node if among is None else among.numel()
    ids, counts = torch.zeros(T, dtype=torch.int64, device=dev), torch.zeros(T, dtype=torch.int32, device=dev)
    nv, nd = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = int(lib.tg_trending_workspace_bytes(n, T))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    g = graph.tcsr

    def run():
        for _ in range(inner):
            check(lib.tg_trending(C.byref(g), t_lo, t_hi, ptr(among), 0 if among is None else n, T, ptr(ids), ptr(counts), ptr(nv),
                                  ptr(nd), ptr(ws), nbytes, hip_ops.stream_ptr(dev)), 'tg_trending')

    run()
    out = stats([timed(run) for _ in range(reps)], inner)
    out.update(eligible=n, workspace_bytes=nbytes, n_distinct=int(nd), top_count=int(counts[0]))
    return out


def fill_call(graph, src, ts, rows, trend, exclude_seen, reps, inner):
    dev = src.device
    B = src.numel()
    ids, counts, nv = rows['ids'].clone(), rows['counts'].clone(), rows['n_valid'].clone()
    n_filled = torch.zeros(B, dtype=torch.int32, device=dev)
    g = graph.tcsr

    def restore():
        for _ in range(inner):
            ids.copy_(rows['ids']), counts.copy_(rows['counts']), nv.copy_(rows['n_valid'])

    def run():
        for _ in range(inner):
            ids.copy_(rows['ids']), counts.copy_(rows['counts']), nv.copy_(rows['n_valid'])
            check(lib.tg_fill_candidates(C.byref(g), B, ptr(src), ptr(ts), CN, ptr(ids), ptr(counts), ptr(nv), ptr(trend['ids']),
                                         ptr(trend['n_valid']), T, 1 if exclude_seen else 0, ptr(n_filled),
                                         hip_ops.stream_ptr(dev)), 'tg_fill_candidates')

    run()
    out = dict(fill_and_restore=stats([timed(run) for _ in range(reps)], inner), restore=stats([timed(restore) for _ in range(reps)], inner))
    out.update(lds_bytes=int(lib.tg_fill_candidates_lds_bytes(T)), mean_walk_valid=round(float(rows['n_valid'].float().mean()), 1),
               mean_filled=round(float(n_filled.float().mean()), 1), full_rows=int((rows['n_valid'] >= CN).sum()))
    return out


def recall(graph, st, items, exclude_seen, n_batches=100):
    dev = graph.device
    walked = covered = n = 0
    E = len(st['src'])
    for lo in range(E - n_batches * BS, E, BS):
        src, dst = (torch.from_numpy(st[k][lo:lo + BS]).to(dev) for k in ('src', 'dst'))
        ts = torch.from_numpy(st['ts'][lo:lo + BS].astype(np.float64)).to(dev)
        rows = hip_ops.walk_candidates(graph, src, ts, CN, fanout=FANOUT, take=TAKE, exclude_seen=exclude_seen)
        trend = hip_ops.trending(graph, float(ts.min()), T, among=items)
        full = hip_ops.fill_candidates(graph, src, ts, rows, trend, exclude_seen=exclude_seen)
        walked += int(((rows['ids'] == dst[:, None]) & (rows['ids'] != 0)).any(1).sum())
        covered += int(((full['ids'] == dst[:, None]) & (full['ids'] != 0)).any(1).sum())
        n += BS
    return dict(exclude_seen=exclude_seen, coverage_walk=round(walked / n, 5), coverage=round(covered / n, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=150, help='batches of 200 events in the stream (the graph covers all of them)')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fill_candidates_v1.json'))
    a = ap.parse_args()
    if a.reps < 30:
        raise SystemExit('--reps: at least 30 samples')
    c = bench.C2
    E = a.batches * BS
    st = bench.make_stream(c['n_u'], c['n_i'], E, c['T'] * E / c['E'], seed=0, d_e=c['d'])
    dev = torch.device('cuda', 0)
    graph = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy='recent_edges', seed=0,
                              max_node_id=st['n_nodes'] - 1, device=dev)
    items = torch.arange(c['n_u'] + 1, c['n_u'] + c['n_i'] + 1, dtype=torch.int64, device=dev)   # all destinations
    p = torch.cuda.get_device_properties(0)
    out = dict(tool='fill_candidates_bench', workload='C2-shaped stream, graph only', device=p.name,
               compute_units=p.multi_processor_count, events=E, C=CN, T=T, fanout=list(FANOUT), take='levels 1 and 3',
               command=' '.join(['python', 'tools/fill_candidates_bench.py'] + sys.argv[1:]), trending=[], fill=[])
    t_hi = float(st['ts'].max()) + 1.0
    span = t_hi - float(st['ts'].min())
    # (a) the stream's destinations; the same events spread over 10^6 node ids (every id a multiple of a stride)
    stride = (BIG_N - 1) // st['n_nodes']
    big = Graph.from_arrays(st['src'] * stride, st['dst'] * stride, st['ts'], st['eids'], strategy='recent_edges', seed=0,
                            max_node_id=BIG_N - 1, device=dev)
    for name, g, among in (('destinations', graph, items), ('10^6 nodes', big, None)):
        for window in (None, span / 10):
            row = dict(case=name, window=None if window is None else round(window, 1),
                       **trending_call(g, -float('inf') if window is None else t_hi - window, t_hi, among, a.reps, a.inner))
            out['trending'].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    # (b) the fill beside the walk
    trend = hip_ops.trending(graph, float(st['ts'][E - 1024]), T, among=items)
    for B in BATCHES:
        src = torch.from_numpy(st['src'][E - B:]).to(dev)
        ts = torch.from_numpy(st['ts'][E - B:].astype(np.float64)).to(dev)
        row = dict(B=B, walk_call=walk_call(graph, src, ts, FANOUT, CN, a.reps, a.inner))
        for ex in (False, True):
            rows = hip_ops.walk_candidates(graph, src, ts, CN, fanout=FANOUT, take=TAKE, exclude_seen=ex)
            row['fill_exclude_seen' if ex else 'fill'] = fill_call(graph, src, ts, rows, trend, ex, a.reps, a.inner)
        out['fill'].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    # (c)
    out['recall_last_100_batches'] = [recall(graph, st, items, ex) for ex in (False, True)]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
