#!/usr/bin/env python3
"""Walk-candidate measurements (one JSON line, also written to profiles/walk_candidates_v1.json) on the C2-shaped synthetic
stream (d = 172, K = 10, 'bin' hits), graph over the whole stream, state warmed by `--warm` streamed batches of 200 events.
Fan-outs (10, 10, 10) and (20, 10, 10), levels 1 and 3 taken; B in (1, 200, 1024) queries taken from the stream's tail.

  (a) walk_call        tg_walk_candidates alone, C = 256, exclude_seen: HIP events around `--inner` back-to-back calls on
                       preallocated outputs after a warm-up call, `--reps` (>= 30) samples, median / min / max per call
  (b) recommend_walk   TIGE.recommend over the walk's [B, C] ids, C in (256, 1000), beside
      recommend_all    TIGE.recommend over the catalogue of all destinations of the stream on the per-pair path - code
                       this tool's subject does not touch, so the baseline.  `--rec_reps` samples each.  The walk's own
                       call is NOT inside recommend_walk's time; (a) gives it.
  (c) recall           the share of the events of the stream's last 100 batches of 200 whose true destination is among
                       the C walk candidates of (source, event time), C in (256, 1000), with and without exclude_seen -
                       the generator alone, no model
Nothing is asserted and there is no threshold; the lists of (b) are not compared (different candidate sets).

    python tools/walk_candidates_bench.py [--reps 30] [--out profiles/walk_candidates_v1.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from www2023tiger_amd import hip_ops  # noqa: E402
from www2023tiger_amd._lib import check, lib, ptr  # noqa: E402

BS = 200
FANOUTS = ((10, 10, 10), (20, 10, 10))
TAKE = (True, False, True)
BATCHES = (1, 200, 1024)
CS = (256, 1000)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms, per=1):
    v = [x / per for x in ms]
    return dict(median_us=round(statistics.median(v) * 1e3, 2), min_us=round(min(v) * 1e3, 2), max_us=round(max(v) * 1e3, 2),
                samples=len(v))


def setup(warm, n_batches):
    c = bench.C2
    E = n_batches * BS
    st = bench.make_stream(c['n_u'], c['n_i'], E, c['T'] * E / c['E'], seed=0, d_e=c['d'])
    model, _ = bench.build_models(st, c['d'], c['K'], c['msg_src'], c['upd_src'], restarter='static', hist_len=20, dropout=0.1)
    model.eval()
    for b in range(warm):
        model.stream_step(*[st[k][b * BS:(b + 1) * BS] for k in ('src', 'dst', 'neg', 'ts', 'eids')])
    return model, st


def walk_call(graph, src, ts, fanout, Cn, reps, inner):
    dev = src.device
    B = src.numel()
    fan = torch.tensor(fanout, dtype=torch.int32)
    bits = sum(1 << l for l, b in enumerate(TAKE) if b)
    ids = torch.zeros(B, Cn, dtype=torch.int64, device=dev)
    counts = torch.zeros(B, Cn, dtype=torch.int32, device=dev)
    nv, nd = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    g = graph.tcsr

    def run():
        for _ in range(inner):
            check(lib.tg_walk_candidates(C.byref(g), B, ptr(src), ptr(ts), 3, ptr(fan), bits, Cn, 1, ptr(ids), ptr(counts),
                                         ptr(nv), ptr(nd), hip_ops.stream_ptr(dev)), 'tg_walk_candidates')

    run()
    out = stats([timed(run) for _ in range(reps)], inner)
    out.update(lds_bytes=int(lib.tg_walk_candidates_lds_bytes(3, ptr(fan), bits)), mean_distinct=round(float(nd.float().mean()), 1),
               max_distinct=int(nd.max()))
    return out


def recall(graph, st, fanout, Cn, exclude_seen, n_batches=100):
    dev = graph.device
    hit = n = 0
    E = len(st['src'])
    for lo in range(E - n_batches * BS, E, BS):
        src, dst = (torch.from_numpy(st[k][lo:lo + BS]).to(dev) for k in ('src', 'dst'))
        ts = torch.from_numpy(st['ts'][lo:lo + BS].astype(np.float64)).to(dev)
        ids = hip_ops.walk_candidates(graph, src, ts, Cn, fanout=fanout, take=TAKE, exclude_seen=exclude_seen)['ids']
        hit += int(((ids == dst[:, None]) & (ids != 0)).any(1).sum())
        n += BS
    return round(hit / n, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=40, help='streamed batches of 200 events before the measurement')
    ap.add_argument('--batches', type=int, default=150, help='batches of 200 events in the stream (the graph covers all of them)')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--rec_reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'walk_candidates_v1.json'))
    a = ap.parse_args()
    if a.reps < 30:
        raise SystemExit('--reps: at least 30 samples')
    model, st = setup(a.warm, a.batches)
    c, dev, graph = bench.C2, model.device, model.graph
    items = torch.arange(c['n_u'] + 1, c['n_u'] + c['n_i'] + 1, dtype=torch.int64, device=dev)   # all destinations
    p = torch.cuda.get_device_properties(0)
    out = dict(tool='walk_candidates_bench', workload="C2-shaped stream, d 172, K 10, 'bin' hits, k 10", device=p.name,
               compute_units=p.multi_processor_count, events=len(st['src']), warm_batches=a.warm, take='levels 1 and 3',
               command=' '.join(['python', 'tools/walk_candidates_bench.py'] + sys.argv[1:]), results=[])
    E = len(st['src'])
    for fanout in FANOUTS:
        for B in BATCHES:
            src = torch.from_numpy(st['src'][E - B:]).to(dev)
            ts = torch.from_numpy(st['ts'][E - B:].astype(np.float64)).to(dev)
            row = dict(fanout=list(fanout), B=B, walk_call=walk_call(graph, src, ts, fanout, 256, a.reps, a.inner))
            for Cn in CS:
                cand = hip_ops.walk_candidates(graph, src, ts, Cn, fanout=fanout, take=TAKE, exclude_seen=True)['ids']
                model.recommend(src, ts, cand, 10)
                row[f'recommend_walk_C{Cn}'] = stats([timed(lambda: model.recommend(src, ts, cand, 10)) for _ in range(a.rec_reps)])
            if fanout == FANOUTS[0]:   # the baseline does not depend on the fan-out
                model.recommend(src, ts, items, 10)
                row['recommend_all_destinations'] = dict(stats([timed(lambda: model.recommend(src, ts, items, 10))
                                                                for _ in range(a.rec_reps)]), C=int(items.numel()))
            out['results'].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        out.setdefault('recall_last_100_batches', []).extend(
            dict(fanout=list(fanout), C=Cn, exclude_seen=ex, recall=recall(graph, st, fanout, Cn, ex)) for Cn in CS for ex in (False, True))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
