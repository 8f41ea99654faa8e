#!/usr/bin/env python3
"""Incremental catalogue refresh, measured (one JSON line, also written to profiles/catalogue_refresh_v1.json): C2-shaped
stream (d = 172, K = 10), a model whose graph and edge table cover the first `--warm` batches of 1 024 events and that has
streamed them, change tracking on, the catalogue = ALL destination nodes (and, in a second pass for comparison, all node
ids: a catalogue of more than one embedding unit).  Then, `--reps` times and alternating between a batch of 200 and a
batch of 1 024 NEW events:

    observe(batch)                                   (not timed: ingestion is not what is measured)
    dirty_pass      hip_ops.catalogue_dirty alone on the tracker's bits (three launches, nothing read back)
    refresh         TIGE.refresh_catalogue(snap, t)  (dirty pass, ONE count read back, n_dirty embeddings, P, merge)
    embed           TIGE.embed_catalogue(items, t)   (the yardstick: all C embeddings, same model, same process, same t)

every call between its own device events after a synchronise; per batch size the median and the 10th - 90th percentile in
microseconds, n_dirty beside every refresh time.  Nothing is asserted and no ratio is promised: the dirty share depends on
the data.  (tests/test_hip_refresh_model.py holds the refreshed rows to the bits of a fresh embedding.)

    python tools/catalogue_refresh_bench.py [--reps 30] [--out profiles/catalogue_refresh_v1.json]
"""
import argparse
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

SIZES = (200, 1024)
WARM_BS = 1024


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    v = sorted(ms)
    q = statistics.quantiles(v, n=10)
    return dict(median_us=round(statistics.median(v) * 1e3, 1), p10_us=round(q[0] * 1e3, 1), p90_us=round(q[-1] * 1e3, 1),
                samples=len(v))


def setup(warm, reps):
    """a C2-shaped model over the first warm * 1 024 events (graph and edge table), which it has streamed"""
    from www2023tiger_amd.data.graph import Graph
    c = bench.C2
    E0 = warm * WARM_BS
    E = E0 + reps * sum(SIZES)
    st = bench.make_stream(c['n_u'], c['n_i'], E, c['T'] * E / c['E'], seed=0, d_e=c['d'])
    model, _ = bench.build_models(st, c['d'], c['K'], c['msg_src'], c['upd_src'], restarter='static', hist_len=20, dropout=0.1)
    model.eval()
    strategy = model.graph.strategy
    model.graph = Graph.from_arrays(*(st[k][:E0] for k in ('src', 'dst', 'ts', 'eids')), strategy=strategy, seed=0,
                                    max_node_id=st['n_nodes'] - 1, device=model.device)
    fg = model.raw_feat_getter
    fg.efeats = fg.efeats[:E0 + 1].clone()
    model.invalidate_struct()
    for b in range(warm):
        model.stream_step(*[st[k][b * WARM_BS:(b + 1) * WARM_BS] for k in ('src', 'dst', 'neg', 'ts', 'eids')])
    return model, st, E0


def measure(model, st, lo, items, reps):
    """reps + 1 rounds (round 0 warms every path up and is dropped) of [observe, dirty pass, refresh, embed] per batch size
    on the catalogue `items`, from event `lo` of the stream on -> (results per batch size, the next event)"""
    dev, tr = model.device, model.track_changes()
    tr.clear()
    t = float(st['ts'][lo - 1])
    snap = model.embed_catalogue(items, t)
    model.recommend(torch.from_numpy(st['src'][:4]).to(dev), torch.full((4,), t, dtype=torch.float64, device=dev), snap, 10)  # P
    rows = {n: dict(dirty_pass=[], refresh=[], embed=[], n_dirty=[]) for n in SIZES}
    for rep in range(reps + 1):
        for n in SIZES:
            s = slice(lo, lo + n)
            lo += n
            model.observe(st['src'][s], st['dst'][s], st['ts'][s], st['eids'][s], efeats=st['efeats'][s.start + 1:s.stop + 1])
            t = float(st['ts'][s][-1])
            t_old = snap.t if snap.t_row is None else snap.t_row
            ms_d, _ = timed(lambda: hip_ops.catalogue_dirty(model.graph, snap.ids, t_old, model.n_neighbors, model.n_layers,
                                                            tr.bits, t, check_ids=False))
            ms_r, child = timed(lambda: model.refresh_catalogue(snap, t))
            ms_e, _ = timed(lambda: model.embed_catalogue(items, t))
            snap = child
            if rep:
                r = rows[n]
                r['dirty_pass'].append(ms_d)
                r['refresh'].append(ms_r)
                r['embed'].append(ms_e)
                r['n_dirty'].append(model.last_refreshed[0])
    out = []
    for n in SIZES:
        r = rows[n]
        nd = r['n_dirty']
        out.append(dict(batch=n, dirty_pass=stats(r['dirty_pass']), refresh=stats(r['refresh']), embed_catalogue=stats(r['embed']),
                        n_dirty=dict(median=int(np.median(nd)), min=int(min(nd)), max=int(max(nd)), per_refresh=nd),
                        refresh_us_per_sample=[round(x * 1e3, 1) for x in r['refresh']]))
    return out, lo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warm', type=int, default=40, help='streamed batches of 1 024 events before the measurement')
    ap.add_argument('--reps', type=int, default=30, help='refreshes per batch size and catalogue')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'catalogue_refresh_v1.json'))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit('--reps: at least 10 samples per batch size')
    model, st, lo = setup(a.warm, 2 * (a.reps + 1))   # (two catalogues, and round 0 of each is a warm-up)
    c, dev = bench.C2, model.device
    p = torch.cuda.get_device_properties(0)
    out = dict(tool='catalogue_refresh_bench', workload='C2-shaped stream, d 172, K 10', device=p.name,
               compute_units=p.multi_processor_count, n_layers=model.n_layers, strategy=model.graph.strategy,
               embed_unit_rows=model.RANK_EMBED_ROWS, warm_events=a.warm * WARM_BS,
               command=' '.join(['python', 'tools/catalogue_refresh_bench.py'] + sys.argv[1:]), catalogues=[])
    # the shape asked for: all destination nodes.  Beside it all node ids: a catalogue of more than one embedding unit
    # (`_embed_queries` embeds in calls of exactly RANK_EMBED_ROWS rows, so a catalogue below one unit costs one unit
    # however few of its rows are dirty)
    for name, items in (('all destination nodes', torch.arange(c['n_u'] + 1, c['n_u'] + c['n_i'] + 1, dtype=torch.int64, device=dev)),
                        ('all node ids', torch.arange(st['n_nodes'], dtype=torch.int64, device=dev))):
        res, lo = measure(model, st, lo, items, a.reps)
        out['catalogues'].append(dict(catalogue=name, C=int(items.numel()), results=res))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
