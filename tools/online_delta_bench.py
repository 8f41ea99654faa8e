#!/usr/bin/env python3
"""Incremental online state files against full saves (one JSON line).

Per shape a model B with the sequence restarter, d = 172, observes `--reps` batches of B = 1 024 events.  After every batch
(with `keep_last`: after `forget(keep_last=)`) two things are timed, wall clock between two device synchronisations:

    delta_save   journal.save(sink): listing, gathers, pack, copies to the host, torch.save;
    full_save    model.save_online(sink) of the same state to the same kind of sink - the parent commit's only way.

The sink counts bytes and keeps nothing, so neither side pays for a disk.  The files are also kept as dicts, and a model C
built on a two-node stub then times

    load         C.load_online(base dict)   (`--reps` times, the same dict);
    apply        C.apply_online_delta(dict) once per delta, in order (`--reps` samples, one per batch).

Shapes: `c2` (Wikipedia-shaped: 9 228 node ids, 157 474 events) and `1m` (1 000 000 node ids, keep_last = 128) at every
graph size of --events_1m with the SAME batches, which is what shows whether the cost of a delta follows the dirty set (D_state,
D_graph, packed entries) or n_nodes / num_entry.  Every row records medians, 10th / 90th percentiles, the bytes of both files and
the dirty counts.  After the last delta C is compared with B (torch.equal on every tensor of online_state()).

    python tools/online_delta_bench.py [--shapes c2,1m] [--events_1m 1000000,4000000] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from idmap_bench import pct  # noqa: E402
from www2023tiger_amd.data.graph import Graph  # noqa: E402

D, B = 172, 1024


class CountingSink:
    """a file object that counts what is written and keeps nothing"""

    def __init__(self):
        self.n = 0

    def write(self, b):
        self.n += len(b)
        return len(b)

    def flush(self):
        pass


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def summary(xs):
    return round(statistics.median(xs), 3), [round(pct(xs, 0.1), 3), round(pct(xs, 0.9), 3)]


def model_on(n_nodes, ev, n_rows, dev, seed=0):
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    from www2023tiger_amd.model.restarters import SeqRestarter
    from www2023tiger_amd.model.tiger import TIGER
    g = Graph.from_arrays(*ev, strategy='recent_edges', seed=0, max_node_id=n_nodes - 1, device=dev)
    torch.manual_seed(seed)
    fg = NumericalFeature(torch.zeros(n_nodes, D), torch.zeros(n_rows, D), dim=D, device=dev)
    rst = SeqRestarter(raw_feat_getter=fg, graph=g, hist_len=7, n_head=2, dropout=0.0)
    m = TIGER(raw_feat_getter=fg, graph=g, restarter=rst, n_neighbors=10, hit_type='bin', n_layers=1, n_head=2, dropout=0.0,
              msg_src='left', upd_src='left').to(dev)
    return m.eval()


def state_equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(state_equal(a[k], b[k]) for k in a)
    return a == b


def tensor_bytes(v):
    if torch.is_tensor(v):
        return v.numel() * v.element_size()
    return sum(tensor_bytes(x) for x in v.values()) if isinstance(v, dict) else 0


def measure(name, n_nodes, E, keep_last, reps, dev, batch_seed=1):
    rs = np.random.RandomState(0)
    ev = (rs.randint(1, n_nodes, E).astype(np.int64), rs.randint(1, n_nodes, E).astype(np.int64),
          np.sort(rs.uniform(0, 1e6, E)), np.arange(1, E + 1, dtype=np.int64))
    model = model_on(n_nodes, ev, E + 1, dev)
    rb = np.random.RandomState(batch_seed)   # the SAME batches at every graph size of a shape
    if keep_last is not None:
        model.forget(keep_last=keep_last)
    J = model.journal()
    import io
    f = io.BytesIO()
    assert J.save(f) == 'base'
    f.seek(0)
    base = torch.load(f, map_location='cpu', weights_only=True)
    del f
    t = {k: [] for k in ('delta_save', 'full_save', 'load', 'apply', 'observe')}
    deltas, sizes, dirty = [], [], []
    for rep in range(-2, reps):      # (negative: warm-up, applied but not recorded)
        s, d_ = rb.randint(1, n_nodes, B).astype(np.int64), rb.randint(1, n_nodes, B).astype(np.int64)
        ts = 1e6 + (rep + 3) * 10.0 + np.sort(rb.uniform(0, 10.0, B))
        rows = model.raw_feat_getter.efeats.shape[0]
        ms_obs, _ = wall(lambda: (model.observe(s, d_, ts, np.arange(rows, rows + B), efeats=torch.zeros(B, D)),
                                  keep_last is not None and model.forget(keep_last=keep_last)))
        sink = CountingSink()
        buf = io.BytesIO()
        ms_delta, kind = wall(lambda: J.save(buf))
        assert kind == 'delta', J.reason
        buf.seek(0)
        st = torch.load(buf, map_location='cpu', weights_only=True)
        deltas.append(st)
        ms_full, _ = wall(lambda: model.save_online(sink))
        if rep >= 0:
            t['observe'].append(ms_obs)
            t['delta_save'].append(ms_delta)
            t['full_save'].append(ms_full)
            sizes.append((buf.getbuffer().nbytes, sink.n))
            dirty.append((int(st['ids'].numel()), int(st['rows'].numel()), int(st['ts'].numel())))
    print(f'{name} E={E}: {reps} batches saved both ways, loading and applying', file=sys.stderr, flush=True)
    stub = (np.array([1]), np.array([1]), np.array([0.0]), np.array([1]))
    C = model_on(2, stub, 2, dev, seed=9)
    for rep in range(-1, reps):
        ms, _ = wall(lambda: C.load_online(base))
        if rep >= 0:
            t['load'].append(ms)
    for i, st in enumerate(deltas):
        ms, _ = wall(lambda: C.apply_online_delta(st))
        if i >= 2:
            t['apply'].append(ms)
    same = state_equal(model.online_state(), C.online_state())
    assert same, 'the model that applied the deltas is not the model that saved them'
    row = dict(shape=name, n_nodes=n_nodes, events_at_start=E, num_entry=int(model.graph.tcsr.num_entry), keep_last=keep_last,
               batch=B, d=D, reps=reps, results_checked=same,
               delta_bytes_median=int(statistics.median(x[0] for x in sizes)), full_bytes_median=int(statistics.median(x[1] for x in sizes)),
               delta_tensor_bytes_median=int(statistics.median(tensor_bytes(x) for x in deltas[2:])),
               D_state_median=int(statistics.median(x[0] for x in dirty)), D_graph_median=int(statistics.median(x[1] for x in dirty)),
               packed_entries_median=int(statistics.median(x[2] for x in dirty)))
    for k, v in t.items():
        row[f'{k}_ms'], row[f'{k}_ms_p10_p90'] = summary(v)
        row[f'{k}_ms_all'] = [round(x, 2) for x in v]   # (in order: a drift over the run shows here)
    row['full_over_delta_save'] = round(row['full_save_ms'] / row['delta_save_ms'], 1)
    row['load_over_apply'] = round(row['load_ms'] / row['apply_ms'], 1)
    row['full_over_delta_bytes'] = round(row['full_bytes_median'] / row['delta_bytes_median'], 1)
    del model, C, deltas, base
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='c2,1m')
    ap.add_argument('--events_1m', default='1000000,4000000', help='graph sizes (events at the start) of the 1 M-node shape')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    rows = []

    def emit():
        out = dict(tool='online_delta_bench', device=torch.cuda.get_device_name(0), timing='wall clock between device synchronisations, ms',
                   results=rows)
        if a.out:
            with open(a.out, 'w') as f:
                f.write(json.dumps(out) + '\n')
        return out
    for shape in a.shapes.split(','):
        if shape == 'c2':
            rows.append(measure('c2', 9228, 157474, None, a.reps, dev))
        elif shape == '1m':
            for E in (int(x) for x in a.events_1m.split(',') if x):
                rows.append(measure('1m', 1_000_000, E, 128, a.reps, dev))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                emit()
            continue
        else:
            raise SystemExit(f'unknown shape {shape!r}')
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        emit()
    print(json.dumps(emit()))


if __name__ == '__main__':
    main()
