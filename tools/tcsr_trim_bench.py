#!/usr/bin/env python3
"""T-CSR trim measurements (one JSON line).

Leg 1, per shape: `Graph.trimmed(before=t_median)` - half of the events dropped by the horizon - on a device-resident
graph against what existed before it for the same result: filtering the device-resident event columns with torch
(`ts >= t`, four boolean gathers) and tg_tcsr_build_device over what is left, into arrays of the exact size.  The two
alternate for `reps` repetitions after warm-up, each call between its own pair of device events (median, 10th / 90th
percentile; both calls contain one read-back: the kept count), and the two results are compared bit for bit.  The cap
has no rebuild to be compared with (a capped graph is no event list), so `trimmed(before=t_median, keep_last=128)` is
timed alone, the same way.  The effective rate is the bytes a trim must move - 32 per kept entry (16 read, 16 written)
and 36 per node (indptr read, shift and rank written and read, indptr_out written) - over the median call time.  Shapes
(those of tools/tcsr_append_bench.py):

    c2    the C2 stream (bench.make_stream: 157 474 events, 9 228 nodes)
    c3    the C3 stream (672 447 events, 10 985 nodes)
    big   10 M events over 1 M nodes, generated on the device (beyond the last-level cache)

Only `big` says anything about HBM bandwidth (peak 8 TB/s); c2 and c3 fit the caches and are bound by their launches and
the read-back.

Leg 2 (--grow): the graph side of `TIGE.observe` for `batches` batches of 200 events on a C2-shaped stream that is long
enough (the model's step does not depend on the size of the graph): `Graph.extended` per batch, with and without
`trimmed(keep_last=128)` every 50 batches; the per-call time of the extension (tg_tcsr_append, between device events) over
the first and over the last 100 batches of each run.  The claim to confirm or refute: flat with forgetting, growing
without.

    python tools/tcsr_trim_bench.py [--shapes c2,c3,big] [--reps 100] [--grow] [--batches 2000] [--out FILE]
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
from tcsr_append_bench import SHAPES, device_stream, out_arrays, pct  # noqa: E402
from www2023tiger_amd._lib import check, lib, ptr  # noqa: E402
from www2023tiger_amd.data.graph import Graph  # noqa: E402
from www2023tiger_amd.hip_ops import stream_ptr  # noqa: E402

KEEP_LAST = 128


def device_graph(ev, N, dev):
    """a device-resident Graph over device-resident event columns (no host copy of the stream is made)"""
    E = ev[0].numel()
    out = out_arrays(N, 2 * E, dev)
    bw = int(lib.tg_tcsr_build_device_workspace_bytes(E, N))
    ws = torch.empty(max(bw, 16), dtype=torch.uint8, device=dev)
    check(lib.tg_tcsr_build_device(E, *(ptr(a) for a in ev), N, *(ptr(a) for a in out), ptr(ws), bw, stream_ptr(dev)), 'build')
    torch.cuda.synchronize()
    return Graph._from_device_arrays(out, float(ev[2][-1]) if E else -np.inf, True, strategy='recent_edges', seed=0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, r


def measure(name, cfg, reps, dev):
    ev, N = device_stream(cfg, dev)
    E = ev[0].numel()
    g = device_graph(ev, N, dev)
    t_cut = float(ev[2][E // 2])
    bw = int(lib.tg_tcsr_build_device_workspace_bytes(E, N))
    ws = torch.empty(max(bw, 16), dtype=torch.uint8, device=dev)
    s = stream_ptr(dev)

    def trim():
        return g.trimmed(before=t_cut)._dev

    def trim_cap():
        return g.trimmed(before=t_cut, keep_last=KEEP_LAST)._dev

    def rebuild():
        m = ev[2] >= t_cut
        kept = tuple(a[m] for a in ev)   # (the first gather reads the kept count back)
        n = kept[0].numel()
        out = out_arrays(N, 2 * n, dev)
        check(lib.tg_tcsr_build_device(n, *(ptr(a) for a in kept), N, *(ptr(a) for a in out), ptr(ws), bw, s), 'rebuild')
        return out
    fns = (('trim', trim), ('rebuild', rebuild), ('trim_cap', trim_cap))
    for _ in range(5):
        got = {k: fn() for k, fn in fns}
    torch.cuda.synchronize()
    for a, b in zip(got['trim'], got['rebuild']):
        assert torch.equal(a, b), 'the trim differs from the rebuild over the filtered events'
    t = {k: [] for k, _ in fns}
    for _ in range(reps):   # alternating, every call between its own events
        for k, fn in fns:
            t[k].append(timed(fn)[0])
    kept, kept_cap = got['trim'][1].numel(), got['trim_cap'][1].numel()
    row = dict(shape=name, events=E, nodes=N, reps=reps, t_cut=t_cut, keep_last=KEEP_LAST, entries=2 * E, entries_kept=kept,
               entries_kept_with_cap=kept_cap, bit_equal_to_rebuild=True)
    for k, _ in fns:
        row[f'{k}_call_us'] = round(statistics.median(t[k]), 2)
        row[f'{k}_call_us_p10_p90'] = [round(pct(t[k], 0.1), 2), round(pct(t[k], 0.9), 2)]
    row['trim_bytes'] = 32 * kept + 36 * N
    row['trim_effective_GBps'] = round(row['trim_bytes'] / statistics.median(t['trim']) / 1e3, 1)
    row['trim_fraction_of_8TBps'] = round(row['trim_effective_GBps'] / 8000.0, 4)
    row['speedup_call'] = round(row['rebuild_call_us'] / row['trim_call_us'], 2)
    row['trim_p90_below_rebuild_p10'] = bool(pct(t['trim'], 0.9) < pct(t['rebuild'], 0.1))
    return [row]


def measure_grow(dev, batches, B=200, every=50, E0=40000):
    cfg = SHAPES['c2']
    E = E0 + batches * B
    st = bench.make_stream(cfg['n_u'], cfg['n_i'], E, cfg['T'] * E / cfg['E'], seed=0, with_efeats=False)
    N = st['n_nodes']
    ev = tuple(torch.from_numpy(st[k]).to(dev) for k in ('src', 'dst', 'ts', 'eids'))
    out = dict(shape='c2-shaped', nodes=N, events_start=E0, batch=B, batches=batches, forget_every=every, keep_last=KEEP_LAST)
    for key in ('never_forgets', 'forgets'):
        g = device_graph(tuple(a[:E0].contiguous() for a in ev), N, dev)
        t, trims = [], []
        for b in range(batches):
            sl = slice(E0 + b * B, E0 + (b + 1) * B)
            batch = tuple(a[sl] for a in ev)
            us, g = timed(lambda: g.extended(*batch, validate=False))
            t.append(us)
            if key == 'forgets' and (b + 1) % every == 0:
                us, g = timed(lambda: g.trimmed(keep_last=KEEP_LAST))
                trims.append(us)
        w = min(100, batches // 2)
        out[key] = dict(append_us_first=round(statistics.median(t[:w]), 2), append_us_last=round(statistics.median(t[-w:]), 2),
                        entries_end=int(g.tcsr.num_entry))
        if trims:
            out[key]['trim_us'] = round(statistics.median(trims), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='c2,c3,big')
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--grow', action='store_true')
    ap.add_argument('--batches', type=int, default=2000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    rows = []
    for sname in [x for x in a.shapes.split(',') if x]:
        rows += measure(sname, SHAPES[sname], a.reps, dev)
    out = dict(tool='tcsr_trim_bench', device=torch.cuda.get_device_name(0), results=rows)
    if a.grow:
        out['grow'] = measure_grow(dev, a.batches)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
