#!/usr/bin/env python3
"""Retrieve-then-rank on a catalogue snapshot, measured (one JSON line, also written to profiles/walk_snapshot_v1.json) on
the stream of tools/walk_candidates_bench.py: C2-shaped (d = 172, K = 10, 'bin' hits), graph over the whole stream, state
warmed by `--warm` streamed batches of 200 events.  B in (1, 200, 1024) sources from the stream's tail, every query at ONE
time t behind the stream's last event; the snapshot holds all destination nodes at t; candidates = the walk's [B, 256] ids
(fan-out (10, 10, 10), levels 1 and 3, exclude_seen).  HIP events, a warm-up call first, median / min / max per call.

  (a) scores_gathered   tg_rank_scores_gathered alone on the operands (b) passes: `--reps` (>= 30) samples of `--inner`
                        back-to-back calls.  Beside the time: the share of the 39.3 T unpacked float32 vector op/s issue
                        rate that 6 d operations per pair come to, and the gathered P-row bytes per second
                        (4 d bytes per pair) - both over ALL B x 256 columns, padding included: a padding column is a
                        masked pair that does the same work.  `real_columns` says how many were candidates.
  (b) recommend_subset  TIGE.recommend_subset(src, ts, snap, 10, ids) on a ready snapshot: B source embeddings, (a), top-k
  (c) embed_catalogue   TIGE.embed_catalogue of all destinations at t - paid once per snapshot, not per batch of queries
  (d) recommend_pairs   the baseline (b) replaces, in the same run: TIGE.recommend(src, ts, ids, 10) on the same [B, 256]
                        ids on the per-pair path, B (1 + 256) embeddings
(b), (c) and (d) read a count back, so each call ends in a synchronise: `--rec_reps` single-call samples each.
Nothing is asserted and there is no threshold; (b) and (d) list the same ids with the same score bits (every query stands
at t; tests/test_hip_walk_snapshot.py holds them to that), so the tool does not compare them again.

    python tools/walk_snapshot_bench.py [--reps 30] [--out profiles/walk_snapshot_v1.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from walk_candidates_bench import TAKE, setup, stats, timed  # noqa: E402
from www2023tiger_amd import hip_ops  # noqa: E402
from www2023tiger_amd._lib import check, lib, ptr  # noqa: E402

FANOUT = (10, 10, 10)
BATCHES = (1, 200, 1024)
CN = 256
ISSUE_RATE = 39.3e12   # unpacked float32 vector operations per second, DESIGN 7.9


def scores_gathered(model, snap, src, ts, ids, reps, inner):
    """(a): the C entry alone, on the operands recommend_subset would pass it"""
    from www2023tiger_amd.model.training import score_struct
    dev, d, K = model.device, model.memory_dim, model.n_neighbors
    B, Cq = ids.shape
    with torch.no_grad():
        model._embed_prepare()
        sp = score_struct(model)
        P = model._snapshot_P(snap, sp)
        err = hip_ops.new_err(dev)
        h_src, nb_src = model._embed_queries(src, ts, model.graph, model.graph.strategy, err)
        hip_ops.raise_if_err(err)
    col = snap.col_of[ids].contiguous()
    scores = torch.empty(B, Cq, dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.tg_rank_scores_gathered_workspace_bytes(B, d, C.byref(sp))), dtype=torch.uint8, device=dev)

    def run():
        for _ in range(inner):
            check(lib.tg_rank_scores_gathered(B, len(snap), Cq, d, K, C.byref(sp), ptr(h_src), ptr(P), ptr(nb_src), ptr(snap.nb),
                                              ptr(src), ptr(snap.ids), ptr(col), ptr(scores), Cq, ptr(ws), ws.numel(),
                                              hip_ops.stream_ptr(dev)), 'tg_rank_scores_gathered')

    run()
    out = stats([timed(run) for _ in range(reps)], inner)
    sec = out['median_us'] * 1e-6
    pairs = B * Cq
    out.update(pairs=pairs, real_columns=int(((col >= 0) & (ids != 0)).sum()), vector_ops=6 * d * pairs, p_row_bytes=4 * d * pairs,
               share_of_issue_rate=round(6 * d * pairs / sec / ISSUE_RATE, 4), p_row_gbytes_per_s=round(4 * d * pairs / sec / 1e9, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=40, help='streamed batches of 200 events before the measurement')
    ap.add_argument('--batches', type=int, default=150, help='batches of 200 events in the stream (the graph covers all of them)')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--rec_reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'walk_snapshot_v1.json'))
    a = ap.parse_args()
    if a.reps < 30:
        raise SystemExit('--reps: at least 30 samples')
    model, st = setup(a.warm, a.batches)
    c, dev, graph = bench.C2, model.device, model.graph
    items = torch.arange(c['n_u'] + 1, c['n_u'] + c['n_i'] + 1, dtype=torch.int64, device=dev)   # all destinations
    when = float(st['ts'].astype(np.float64).max()) + 1.0
    p = torch.cuda.get_device_properties(0)
    out = dict(tool='walk_snapshot_bench', workload="C2-shaped stream, d 172, K 10, 'bin' hits, k 10", device=p.name,
               compute_units=p.multi_processor_count, events=len(st['src']), warm_batches=a.warm, fanout=list(FANOUT),
               take='levels 1 and 3', C=CN, catalogue=int(items.numel()), issue_rate_ops_per_s=ISSUE_RATE,
               command=' '.join(['python', 'tools/walk_snapshot_bench.py'] + sys.argv[1:]), results=[])
    model.embed_catalogue(items, when)
    out['embed_catalogue'] = stats([timed(lambda: model.embed_catalogue(items, when)) for _ in range(a.rec_reps)])
    snap = model.embed_catalogue(items, when)
    E = len(st['src'])
    for B in BATCHES:
        src = torch.from_numpy(st['src'][E - B:]).to(dev)
        ts = torch.full((B,), when, dtype=torch.float64, device=dev)
        ids = hip_ops.walk_candidates(graph, src, ts, CN, fanout=FANOUT, take=TAKE, exclude_seen=True)['ids']
        row = dict(B=B, scores_gathered=scores_gathered(model, snap, src, ts, ids, a.reps, a.inner))
        model.recommend_subset(src, ts, snap, 10, ids)
        row['recommend_subset'] = stats([timed(lambda: model.recommend_subset(src, ts, snap, 10, ids)) for _ in range(a.rec_reps)])
        model.recommend(src, ts, ids, 10)
        row['recommend_pairs'] = stats([timed(lambda: model.recommend(src, ts, ids, 10)) for _ in range(a.rec_reps)])
        out['results'].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
