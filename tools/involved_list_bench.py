#!/usr/bin/env python3
"""Involved-list measurements (one JSON line): tg_involved_list over a flat list of (node, time) queries against the path
that produced the same set before it - GraphCollator.collate_memory_nodes (the sampler's [Q, K] and, with two layers,
[Q K, K] neighbour / edge-id / time arrays, written and thrown away) followed by unique_compact.  On the C2 stream
(bench.make_stream: 157 474 events, 9 228 nodes), K = 10, one and two layers, at two query shapes:

    recommend   B = 200 events, a catalogue of 1 000 items: Q = 200 * 1 002 queries (sources, destinations, candidates)
    rank        B = 1 024 events, 100 candidates each:      Q = 1 024 * 102

Queries are the events behind 90 % of the stream with random item candidates, each at its event's time.  Both paths are
timed in one process, alternating, each repetition between its own pair of device events after warm-up (median, 10th /
90th percentile of >= 20 repetitions), with the peak of torch's allocator over one call of each (outputs and workspace
included).  The new entry starts from an empty up-to-date bitmap every time, so it lists the whole set, as the old path
does; the two lists are compared, id for id, before anything is timed.

    python tools/involved_list_bench.py [--reps 30] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from www2023tiger_amd import hip_ops  # noqa: E402
from www2023tiger_amd.data.data_loader import GraphCollator  # noqa: E402
from www2023tiger_amd.data.graph import Graph  # noqa: E402

C2 = dict(n_u=8227, n_i=1000, E=157474, T=2.68e6)
SHAPES = {'recommend': (200, 1000), 'rank': (1024, 100)}
K = 10


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def queries(st, B, C, dev):
    """sources, destinations and C item candidates of B events behind 90 % of the stream, each at its event's time"""
    lo = int(0.9 * len(st['src']))
    src, dst, ts = st['src'][lo:lo + B], st['dst'][lo:lo + B], st['ts'][lo:lo + B]
    cand = np.random.RandomState(0).randint(C2['n_u'] + 1, st['n_nodes'], (B, C)).astype(np.int64)
    nodes = np.concatenate([src, np.concatenate([dst[:, None], cand], 1).ravel()])
    times = np.concatenate([ts, np.repeat(ts, C + 1)])
    return torch.from_numpy(nodes).to(dev), torch.from_numpy(times).to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def measure(g, st, shape, L, reps, dev):
    B, C = SHAPES[shape]
    nodes, times = queries(st, B, C, dev)
    Q, n_nodes = nodes.numel(), st['n_nodes']
    coll = GraphCollator(g, K, L)

    def new():
        bm = hip_ops.new_bitmap(n_nodes, dev)
        return hip_ops.involved_list(g, nodes, times, K, L, bm)

    def old():
        return coll.collate_memory_nodes(nodes, times)[2]

    a, b = new(), old()
    n = int(a['count'].item())
    assert n == int(b['count'].item()) and torch.equal(a['ids'][:n], b['ids'][:n]), 'the two paths list different sets'
    del a, b
    for _ in range(5):
        new()
        old()
    torch.cuda.synchronize()
    t = {'involved_list': [], 'collate_compact': []}
    for _ in range(reps):   # alternating, every call between its own events
        t['involved_list'].append(timed(new))
        t['collate_compact'].append(timed(old))
    row = dict(shape=shape, events=B, candidates=C, queries=Q, n_layers=L, K=K, nodes=n_nodes, involved=n, reps=reps)
    for key, fn in (('involved_list', new), ('collate_compact', old)):
        row[f'{key}_us'] = round(statistics.median(t[key]), 1)
        row[f'{key}_us_p10_p90'] = [round(pct(t[key], 0.1), 1), round(pct(t[key], 0.9), 1)]
        row[f'{key}_peak_bytes'] = peak_bytes(fn)
    row['workspace_bytes'] = int(hip_ops.lib.tg_involved_list_workspace_bytes(n_nodes, Q, K, L))
    row['speedup'] = round(row['collate_compact_us'] / row['involved_list_us'], 2)
    row['involved_list_p90_below_collate_p10'] = bool(pct(t['involved_list'], 0.9) < pct(t['collate_compact'], 0.1))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert a.reps >= 20, 'medians of at least 20 repetitions'
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    st = bench.make_stream(C2['n_u'], C2['n_i'], C2['E'], C2['T'], seed=0, with_efeats=False)
    g = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy='recent_edges', max_node_id=st['n_nodes'] - 1,
                          device=dev)
    rows = [measure(g, st, shape, L, a.reps, dev) for shape in SHAPES for L in (1, 2)]
    line = json.dumps(dict(tool='involved_list_bench', device=torch.cuda.get_device_name(0), stream='c2', results=rows))
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
