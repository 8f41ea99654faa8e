#!/usr/bin/env python3
"""Edge-row release measurements (one JSON line).

Leg 1, per shape: a device-resident graph trimmed to every node's last 128 entries and the edge table of its whole stream
(E + 1 rows of d_e = 172 floats); what `TIGE.release_edge_rows` runs on them - `NumericalFeature.compact_edge_rows` (plan,
one read-back, allocation with head-room, apply) and `Graph.renumbered` - against the same result in torch on the same
device-resident arrays: `torch.unique` of the masked eids (with row 0), `index_select` of the rows, `searchsorted` for the
new ids, bit 31 carried over.  (The torch formulation builds no remap for the caller's pending eids; the release does.)
The two results are compared bit for bit, then the two alternate for `reps` repetitions after warm-up, each call between
its own pair of device events (median, 10th / 90th percentile; both contain one read-back: the live count).  The
effective rate of the CALL is the bytes a release must move - 8 d_e per live row (read, written), 8 per entry (the remap
pass: eid read, eid written) and 3 per table row for the marks (zeroed, read by both scan launches) - over the median
call time; the mark pass's own read of the eids, the remap gathers and the inverse list are not counted.
Shapes (those of tools/tcsr_trim_bench.py):

    c2    the C2 stream (bench.make_stream: 157 474 events, 9 228 nodes)
    c3    the C3 stream (672 447 events, 10 985 nodes)
    big   10 M events over 1 M nodes, generated on the device (a 6.9 GB table: beyond the last-level cache)

Only `big` says anything about HBM bandwidth (peak 8 TB/s); c2 and c3 are bound by their launches and the read-back.

Leg 2 (--grow): the graph and table side of `TIGE.observe` for `batches` batches of 200 events on a C2-shaped stream with
d_e = 172 (`append_edge_rows` + `Graph.extended` per batch; the model's step does not depend on the size of either),
`trimmed(keep_last=128)` every 50 batches, with and without the release behind it: table rows and bytes at the end of both
runs (counts), the median time of the release, the median per-batch time over the first and the last 100 batches.

    python tools/edge_rows_bench.py [--shapes c2,c3,big] [--reps 100] [--grow] [--batches 2000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from tcsr_append_bench import SHAPES, device_stream, pct  # noqa: E402
from tcsr_trim_bench import KEEP_LAST, device_graph, timed  # noqa: E402
from www2023tiger_amd.model.feature_getter import NumericalFeature  # noqa: E402

D_E = 172


def bytes_of(n_live, num_entry, n_rows, d_e):
    """what a release must move: every live row read and written, every eid read and written by the remap pass, the marks
    zeroed once and read by both scan launches"""
    return dict(rows=8 * d_e * n_live, entries=8 * num_entry, marks=3 * n_rows)


def measure(name, cfg, reps, dev):
    ev, N = device_stream(cfg, dev)
    E = ev[0].numel()
    g = device_graph(ev, N, dev).trimmed(keep_last=KEEP_LAST)
    del ev
    gen = torch.Generator(device=dev).manual_seed(1)
    table = torch.randn(E + 1, D_E, generator=gen, device=dev)
    fg = NumericalFeature(None, table[:1], D_E).to(dev)
    fg.efeats = table
    eid = g._tensors()[3]
    zero = torch.zeros(1, dtype=torch.int64, device=dev)

    def release():
        res = fg.compact_edge_rows(g, swap=False)
        return res._store[:res.rows], g.renumbered(res.remap, res.eid_out)._dev[3]

    def in_torch():
        ids = (eid & 0x7FFFFFFF).long()
        live = torch.unique(torch.cat([zero, ids]))   # sorted; reads the live count back
        return table.index_select(0, live), torch.searchsorted(live, ids).int() | (eid & -0x80000000)
    fns = (('release', release), ('torch', in_torch))
    for _ in range(3):
        got = {k: fn() for k, fn in fns}
    torch.cuda.synchronize()
    for a, b in zip(got['release'], got['torch']):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), 'the release differs from torch'
    n_live = got['release'][0].shape[0]
    del got
    t = {k: [] for k, _ in fns}
    for _ in range(reps):   # alternating, every call between its own events
        for k, fn in fns:
            t[k].append(timed(fn)[0])
    P = eid.numel()
    row = dict(shape=name, events=E, nodes=N, reps=reps, keep_last=KEEP_LAST, d_e=D_E, entries=P, rows_before=E + 1,
               rows_live=n_live, table_bytes_before=4 * D_E * (E + 1), table_bytes_after=4 * D_E * n_live, bit_equal_to_torch=True)
    for k, _ in fns:
        row[f'{k}_call_us'] = round(statistics.median(t[k]), 2)
        row[f'{k}_call_us_p10_p90'] = [round(pct(t[k], 0.1), 2), round(pct(t[k], 0.9), 2)]
    b = bytes_of(n_live, P, E + 1, D_E)
    row['release_bytes'] = sum(b.values())
    row['release_effective_GBps'] = round(row['release_bytes'] / statistics.median(t['release']) / 1e3, 1)
    row['release_fraction_of_8TBps'] = round(row['release_effective_GBps'] / 8000.0, 4)
    row['speedup_call'] = round(row['torch_call_us'] / row['release_call_us'], 2)
    row['release_p90_below_torch_p10'] = bool(pct(t['release'], 0.9) < pct(t['torch'], 0.1))
    return [row]


def measure_grow(dev, batches, B=200, every=50, E0=40000):
    cfg = SHAPES['c2']
    E = E0 + batches * B
    st = bench.make_stream(cfg['n_u'], cfg['n_i'], E, cfg['T'] * E / cfg['E'], seed=0, with_efeats=False)
    N = st['n_nodes']
    ev = tuple(torch.from_numpy(st[k]).to(dev) for k in ('src', 'dst', 'ts', 'eids'))
    gen = torch.Generator(device=dev).manual_seed(2)
    first = torch.randn(E0 + 1, D_E, generator=gen, device=dev)
    rows = torch.randn(B, D_E, generator=gen, device=dev)   # (the same rows for every batch: their values do not matter)
    out = dict(shape='c2-shaped', nodes=N, events_start=E0, batch=B, batches=batches, forget_every=every, keep_last=KEEP_LAST,
               d_e=D_E)
    for key in ('forgets', 'forgets_and_releases'):
        g = device_graph(tuple(a[:E0].contiguous() for a in ev), N, dev)
        fg = NumericalFeature(None, first.clone(), D_E).to(dev)
        shift, t, rel, peak = 0, [], [], 0
        for b in range(batches):
            sl = slice(E0 + b * B, E0 + (b + 1) * B)
            s, d, ts, e = (a[sl] for a in ev)
            e = e - shift   # the caller's pending eids

            def step():
                fg.append_edge_rows(rows)
                return g.extended(s, d, ts, e, validate=False)
            us, g = timed(step)
            t.append(us)
            peak = max(peak, fg.efeats.shape[0])
            if (b + 1) % every == 0:
                g = g.trimmed(keep_last=KEEP_LAST)
                if key == 'forgets_and_releases':
                    def release():
                        res = fg.compact_edge_rows(g)
                        return res, g.renumbered(res.remap, res.eid_out)
                    us, (res, g) = timed(release)
                    rel.append(us)
                    shift += res.shift
        w = min(100, batches // 2)
        n = fg.efeats.shape[0]
        out[key] = dict(observe_us_first=round(statistics.median(t[:w]), 2), observe_us_last=round(statistics.median(t[-w:]), 2),
                        entries_end=int(g.tcsr.num_entry), table_rows_end=n, table_bytes_end=4 * D_E * n,
                        backing_rows_end=int(fg._ef_store.shape[0]), backing_bytes_end=4 * D_E * int(fg._ef_store.shape[0]),
                        table_rows_peak=peak)
        if rel:
            out[key]['release_us'] = round(statistics.median(rel), 2)
            out[key]['release_us_p10_p90'] = [round(pct(rel, 0.1), 2), round(pct(rel, 0.9), 2)]
            out[key]['releases'] = len(rel)
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
        torch.cuda.empty_cache()
    out = dict(tool='edge_rows_bench', device=torch.cuda.get_device_name(0), results=rows)
    if a.grow:
        out['grow'] = measure_grow(dev, a.batches)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
