#!/usr/bin/env python3
"""T-CSR extension measurements (one JSON line): tg_tcsr_append of n new events onto a device-resident graph of E0 events
against what was there before it - tg_tcsr_build_device over all E0 + n events, already resident on the device (generous
to the rebuild: a caller would also concatenate and upload them).  Both are timed in one process, alternating, each
repetition between its own pair of device events after warm-up (median, 10th / 90th percentile); `queued_us` is the time
per call of `reps` calls enqueued back to back between one pair of events - launch gaps overlap there, so it is the
closer bound of the kernels' own time - and the effective rate is the bytes the extension must move,
32 * 2 E0 + 56 * n (every old entry read and written once: 16 + 16 bytes; a new event read as 32 bytes and written as
two entries, less the old indptr), over that time.  Shapes:

    c2    the C2 stream (bench.make_stream: 157 474 events, 9 228 nodes), E0 = 90 %, n = 200 and 1 024
    c3    the C3 stream (672 447 events, 10 985 nodes),                    E0 = 90 %, n = 4 096
    big   10 M events over 1 M nodes, generated on the device (320 MB of arrays: beyond the last-level cache), n = 65 536

Only `big` says anything about HBM bandwidth; c2 and c3 fit the caches and are bound by their launches.  With --observe
the tool also times TIGE.observe against TIGE.stream_step on twin C2 models, batch by batch (host clock around a device
synchronise), 200 events each.  Every timed extension is compared with the rebuild, bit for bit.

    python tools/tcsr_append_bench.py [--shapes c2,c3,big] [--reps 100] [--observe] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from www2023tiger_amd._lib import TgTcsr, check, lib, ptr  # noqa: E402
from www2023tiger_amd.hip_ops import stream_ptr, tcsr_arrays as out_arrays  # noqa: E402

SHAPES = {
    'c2': dict(n_u=8227, n_i=1000, E=157474, T=2.68e6, appends=(200, 1024)),
    'c3': dict(n_u=10000, n_i=984, E=672447, T=2.68e6, appends=(4096,)),
    'big': dict(n_nodes=1000000, E=10000000, appends=(65536,)),
}


def device_stream(cfg, dev):
    """(src, dst, ts, eids) on the device, time ordered, and the number of node ids"""
    if 'n_nodes' in cfg:   # too long for the host generator: uniform endpoints, sorted uniform times, seeded
        g = torch.Generator(device=dev).manual_seed(0)
        N, E = cfg['n_nodes'], cfg['E']
        src = torch.randint(1, N, (E,), generator=g, device=dev)
        dst = torch.randint(1, N, (E,), generator=g, device=dev)
        ts = torch.sort(torch.rand(E, generator=g, device=dev, dtype=torch.float64) * 1e8).values.floor()
        return (src, dst, ts, torch.arange(1, E + 1, device=dev)), N
    st = bench.make_stream(cfg['n_u'], cfg['n_i'], cfg['E'], cfg['T'], seed=0, with_efeats=False)
    return tuple(torch.from_numpy(st[k]).to(dev) for k in ('src', 'dst', 'ts', 'eids')), st['n_nodes']


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def measure(name, cfg, reps, dev):
    ev, N = device_stream(cfg, dev)
    E = ev[0].numel()
    s = stream_ptr(dev)
    rows = []
    for n in cfg['appends']:
        E0 = int(0.9 * E)
        old, new, both = (tuple(a[:E0] for a in ev), tuple(a[E0:E0 + n].contiguous() for a in ev),
                          tuple(a[:E0 + n] for a in ev))
        parent = out_arrays(N, 2 * E0, dev)
        bw = int(lib.tg_tcsr_build_device_workspace_bytes(E0 + n, N))
        ws_b = torch.empty(max(bw, 16), dtype=torch.uint8, device=dev)
        check(lib.tg_tcsr_build_device(E0, *(ptr(a) for a in old), N, *(ptr(a) for a in parent), ptr(ws_b), bw, s), 'build')
        g = TgTcsr(N, 2 * E0, *(ptr(a) for a in parent))
        aw = int(lib.tg_tcsr_append_workspace_bytes(2 * E0, n, N))
        ws_a = torch.empty(max(aw, 16), dtype=torch.uint8, device=dev)
        got, want = out_arrays(N, 2 * (E0 + n), dev), out_arrays(N, 2 * (E0 + n), dev)

        def append():
            check(lib.tg_tcsr_append(C.byref(g), n, *(ptr(a) for a in new), *(ptr(a) for a in got), ptr(ws_a), aw, s), 'append')

        def rebuild():
            check(lib.tg_tcsr_build_device(E0 + n, *(ptr(a) for a in both), N, *(ptr(a) for a in want), ptr(ws_b), bw, s),
                  'rebuild')
        for _ in range(5):
            append()
            rebuild()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), 'the extension differs from the rebuild'
        t = {'append': [], 'rebuild': []}
        for _ in range(reps):   # alternating, every call between its own events
            for key, fn in (('append', append), ('rebuild', rebuild)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                t[key].append(a.elapsed_time(b) * 1e3)
        queued = {}
        for key, fn in (('append', append), ('rebuild', rebuild)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            queued[key] = a.elapsed_time(b) * 1e3 / reps
        nbytes = 32 * 2 * E0 + 56 * n
        row = dict(shape=name, events_old=E0, events_new=n, nodes=N, reps=reps, bytes_per_call=nbytes)
        for key in ('append', 'rebuild'):
            row[f'{key}_call_us'] = round(statistics.median(t[key]), 2)
            row[f'{key}_call_us_p10_p90'] = [round(pct(t[key], 0.1), 2), round(pct(t[key], 0.9), 2)]
            row[f'{key}_queued_us'] = round(queued[key], 2)
        row['append_effective_GBps_over_queued_time'] = round(nbytes / queued['append'] / 1e3, 1)
        row['speedup_call'] = round(row['rebuild_call_us'] / row['append_call_us'], 2)
        row['append_p90_below_rebuild_p10'] = bool(pct(t['append'], 0.9) < pct(t['rebuild'], 0.1))
        rows.append(row)
    return rows


def measure_observe(dev, batches=60, B=200):
    """host clock around a synchronise, batch by batch: stream_step on the full graph, observe on a graph that grows"""
    from www2023tiger_amd.data.graph import Graph
    cfg = SHAPES['c2']
    st = bench.make_stream(cfg['n_u'], cfg['n_i'], cfg['E'], cfg['T'], seed=0, d_e=172)
    E0 = int(0.9 * cfg['E'])
    models = []
    for _ in range(2):
        m, _ = bench.build_models(st, d=172, K=10, msg_src='left', upd_src='right', device=str(dev))
        m.fuse_attention()
        m.eager_updates()
        models.append(m)
    A, Bm = models
    Bm.graph = Graph.from_arrays(*(st[k][:E0] for k in ('src', 'dst', 'ts', 'eids')), strategy='recent_edges', seed=0,
                                 max_node_id=st['n_nodes'] - 1, device=dev)
    dv = {k: torch.from_numpy(st[k]).to(dev) for k in ('src', 'dst', 'neg', 'ts', 'eids')}
    t = {'stream_step': [], 'observe': []}
    for b in range(batches + 10):
        sl = slice(E0 + b * B, E0 + (b + 1) * B)
        args = [dv[k][sl] for k in ('src', 'dst', 'neg', 'ts', 'eids')]
        for key in ('stream_step', 'observe'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if key == 'observe':
                Bm.observe(args[0], args[1], args[3], args[4], neg=args[2])
            else:
                A.stream_step(*args)
            torch.cuda.synchronize()
            if b >= 10:
                t[key].append((time.perf_counter() - t0) * 1e6)
    assert torch.equal(A.left_memory.vals, Bm.left_memory.vals), 'observe left another state than stream_step'
    return dict(shape='c2', batch=B, batches=batches, events_old=E0,
                stream_step_us=round(statistics.median(t['stream_step']), 1),
                stream_step_us_p10_p90=[round(pct(t['stream_step'], 0.1), 1), round(pct(t['stream_step'], 0.9), 1)],
                observe_us=round(statistics.median(t['observe']), 1),
                observe_us_p10_p90=[round(pct(t['observe'], 0.1), 1), round(pct(t['observe'], 0.9), 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='c2,c3,big')
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--observe', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    rows = []
    for sname in a.shapes.split(','):
        rows += measure(sname, SHAPES[sname], a.reps, dev)
    out = dict(tool='tcsr_append_bench', device=torch.cuda.get_device_name(0), results=rows)
    if a.observe:
        out['observe'] = measure_observe(dev)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
