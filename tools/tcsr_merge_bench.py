#!/usr/bin/env python3
"""Late-event measurements (one JSON line): tg_tcsr_merge of n late events into a device-resident graph of E0 events against
tg_tcsr_append of n on-time events onto the same graph - the yardstick: both move the same bytes of old entries through the
same apply launch, so what the merge costs beyond it is its sort by (owner, time, j) and its in-row searches.  The late
batch holds times drawn uniformly from the last 10 % of the graph's time range, endpoints drawn from the stream's own events
(its degree distribution), in no order.  `merge_ontime` is the merge given the append's batch: the same sort passes, cut
points at the row ends - the difference to `merge` is what late cut points cost (the searches, and new entries scattered
through the copy tiles instead of standing at row ends).

All three are timed in one process, alternating, each repetition between its own pair of device events after warm-up
(median, 10th / 90th percentile); `queued_us` is the time per call of `reps` calls enqueued back to back between one pair
of events - launch gaps overlap there.  Shapes: those of tools/tcsr_append_bench.py (c2, c3, big), E0 = 90 % of the stream,
n = 200 / 1 024 / 8 192 (2 n = 16 384 entries: past the one-workgroup sort, three radix sorts).  Checked at every timed
size: merge_ontime equals the append bit for bit; the late merge passes tg_tcsr_verify and, on c2 and c3, equals the host
twin bit for bit.

    python tools/tcsr_merge_bench.py [--shapes c2,c3,big] [--reps 100] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcsr_append_bench import SHAPES, device_stream, pct  # noqa: E402
from www2023tiger_amd import hip_ops  # noqa: E402
from www2023tiger_amd._lib import TgTcsr, check, lib, ptr  # noqa: E402
from www2023tiger_amd.hip_ops import stream_ptr, tcsr_arrays as out_arrays  # noqa: E402

BATCHES = (200, 1024, 8192)
KINDS = ('append', 'merge_ontime', 'merge')


def late_batch(ev, E0, n, dev):
    """n late events: endpoints of events drawn from the old stream, times uniform in the last 10 % of its range, new eids"""
    g = torch.Generator(device=dev).manual_seed(n)
    pick = torch.randint(0, E0, (n,), generator=g, device=dev)
    t0, t1 = float(ev[2][0]), float(ev[2][E0 - 1])
    ts = (t1 - 0.1 * (t1 - t0) + torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 0.1 * (t1 - t0)).floor()
    return ev[0][pick].contiguous(), ev[1][pick].contiguous(), ts, torch.arange(1, n + 1, device=dev)


def measure(name, cfg, reps, dev):
    ev, N = device_stream(cfg, dev)
    E = ev[0].numel()
    E0 = int(0.9 * E)
    s = stream_ptr(dev)
    parent = out_arrays(N, 2 * E0, dev)
    bw = int(lib.tg_tcsr_build_device_workspace_bytes(E0, N))
    ws_b = torch.empty(max(bw, 16), dtype=torch.uint8, device=dev)
    check(lib.tg_tcsr_build_device(E0, *(ptr(a[:E0]) for a in ev), N, *(ptr(a) for a in parent), ptr(ws_b), bw, s), 'build')
    g = TgTcsr(N, 2 * E0, *(ptr(a) for a in parent))
    rows = []
    for n in BATCHES:
        ontime, late = tuple(a[E0:E0 + n].contiguous() for a in ev), late_batch(ev, E0, n, dev)
        aw = int(lib.tg_tcsr_append_workspace_bytes(2 * E0, n, N))
        mw = int(lib.tg_tcsr_merge_workspace_bytes(2 * E0, n, N, N))
        ws = torch.empty(max(aw, mw, 16), dtype=torch.uint8, device=dev)
        out = {k: out_arrays(N, 2 * (E0 + n), dev) for k in KINDS}

        def append():
            check(lib.tg_tcsr_append(C.byref(g), n, *(ptr(a) for a in ontime), *(ptr(a) for a in out['append']), ptr(ws), aw, s),
                  'append')

        def merge_ontime():
            check(lib.tg_tcsr_merge(C.byref(g), N, n, *(ptr(a) for a in ontime), *(ptr(a) for a in out['merge_ontime']), ptr(ws),
                                    mw, s), 'merge (on-time batch)')

        def merge():
            check(lib.tg_tcsr_merge(C.byref(g), N, n, *(ptr(a) for a in late), *(ptr(a) for a in out['merge']), ptr(ws), mw, s),
                  'merge')
        fns = dict(append=append, merge_ontime=merge_ontime, merge=merge)
        for _ in range(5):
            for k in KINDS:
                fns[k]()
        torch.cuda.synchronize()
        for a, b in zip(out['merge_ontime'], out['append']):
            assert torch.equal(a, b), 'the merge of an on-time batch differs from the append'
        assert hip_ops.tcsr_verify(out['merge'])[0] == 0, 'the merged graph is no T-CSR'
        checked = 'verify'
        if name != 'big':   # the host twin over the downloaded parent
            h = tuple(np.ascontiguousarray(a.cpu().numpy()) for a in parent)
            b = tuple(np.ascontiguousarray(a.cpu().numpy()) for a in late)
            want = out_arrays(N, 2 * (E0 + n))
            gh = TgTcsr(N, 2 * E0, *(ptr(a) for a in h))
            check(lib.tg_tcsr_merge_host(C.byref(gh), N, n, *(ptr(a) for a in b), *(ptr(a) for a in want)), 'merge_host')
            for a, w in zip(out['merge'], want):
                assert torch.equal(a.cpu(), torch.from_numpy(w)), 'the device merge differs from the host twin'
            checked = 'verify + host twin'
        t = {k: [] for k in KINDS}
        for _ in range(reps):   # alternating, every call between its own events
            for k in KINDS:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fns[k]()
                b.record()
                b.synchronize()
                t[k].append(a.elapsed_time(b) * 1e3)
        queued = {}
        for k in KINDS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fns[k]()
            b.record()
            b.synchronize()
            queued[k] = a.elapsed_time(b) * 1e3 / reps
        row = dict(shape=name, events_old=E0, events_new=n, nodes=N, reps=reps, bytes_per_call=32 * 2 * E0 + 56 * n,
                   sort='one workgroup' if 2 * n <= 4096 else 'three radix sorts', late_merge_checked_by=checked)
        for k in KINDS:
            row[f'{k}_call_us'] = round(statistics.median(t[k]), 2)
            row[f'{k}_call_us_p10_p90'] = [round(pct(t[k], 0.1), 2), round(pct(t[k], 0.9), 2)]
            row[f'{k}_queued_us'] = round(queued[k], 2)
        row['merge_over_append_call'] = round(row['merge_call_us'] / row['append_call_us'], 2)
        row['merge_over_append_queued'] = round(queued['merge'] / queued['append'], 2)
        row['merge_ontime_over_append_queued'] = round(queued['merge_ontime'] / queued['append'], 2)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='c2,c3,big')
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    rows = []
    for sname in a.shapes.split(','):
        rows += measure(sname, SHAPES[sname], a.reps, dev)
    line = json.dumps(dict(tool='tcsr_merge_bench', device=torch.cuda.get_device_name(0), results=rows))
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
