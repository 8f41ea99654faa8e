#!/usr/bin/env python3
"""T-CSR erase measurements (one JSON line).

Per shape, on one device-resident graph, three legs for each of three erasures - a random 1 % of the nodes, a random
50 % of the nodes, a random 1 % of the eids:

    without   `Graph.without(nodes=...)` / `Graph.without(eids=...)`: two bitmap marks, the plan over tiles of the old
              entries, ONE int64 read back, the copy (tg_erase.hip);
    trimmed   `Graph.trimmed(before=t)` with the horizon that keeps about as many entries - the compaction this project
              already had, which keeps a suffix of every row and cannot express an erasure: the yardstick for what moving
              that many entries costs;
    today     the only route to the same result without `without`: download the event columns, filter them on the host
              (numpy isin), `Graph.from_arrays` over what is left, build on the device.

`without` and `trimmed` alternate for `reps` repetitions after warm-up, each call between its own pair of device events
(median, 10th / 90th percentile; both contain one read-back).  `today` is timed with a host clock around a device
synchronise, `reps_today` times (it is host work: seconds at the large shape).  The `without` result is compared bit for
bit with today's route.  The effective rate is the bytes an erase must move - per OLD entry 4 (its neighbour) with nodes
and 4 (its eid) with eids, a quarter byte of keep bits (written once, read once), per KEPT entry 32 (16 read, 16 written),
per node 24 (indptr read twice, indptr_out written) - over the median call time.  Shapes (those of
tools/tcsr_append_bench.py):

    c2    the C2 stream (bench.make_stream: 157 474 events, 9 228 nodes)
    c3    the C3 stream (672 447 events, 10 985 nodes)
    big   10 M events over 1 M nodes, generated on the device (beyond the last-level cache)

Only `big` says anything about HBM bandwidth (peak 8 TB/s); c2 and c3 fit the caches and are bound by their launches and
the read-back.

    python tools/tcsr_erase_bench.py [--shapes c2,c3,big] [--reps 100] [--reps_today 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcsr_append_bench import SHAPES, device_stream, pct  # noqa: E402
from tcsr_trim_bench import device_graph, timed  # noqa: E402
from www2023tiger_amd.data.graph import Graph  # noqa: E402


def erasures(ev, N, seed=0):
    """name -> (nodes or None, eids or None) as device tensors"""
    g = torch.Generator(device=ev[0].device).manual_seed(seed)
    perm = 1 + torch.randperm(N - 1, generator=g, device=ev[0].device)   # never the padding id 0
    E = ev[0].numel()
    eids = ev[3][torch.randperm(E, generator=g, device=ev[0].device)[:max(1, E // 100)]]
    return {'nodes_1pct': (perm[:max(1, N // 100)].contiguous(), None), 'nodes_50pct': (perm[:N // 2].contiguous(), None),
            'eids_1pct': (None, eids.contiguous())}


def today(ev, N, nodes, eids, dev):
    """download, host filter, from_arrays, build on the device -> the device arrays"""
    src, dst, ts, eid = (a.cpu().numpy() for a in ev)
    m = np.ones(len(src), dtype=bool)
    if nodes is not None:
        S = nodes.cpu().numpy()
        m &= ~np.isin(src, S) & ~np.isin(dst, S)
    if eids is not None:
        m &= ~np.isin(eid, eids.cpu().numpy())
    g = Graph.from_arrays(src[m], dst[m], ts[m], eid[m], strategy='recent_edges', seed=0, max_node_id=N - 1, device=dev)
    out = g._tensors()
    torch.cuda.synchronize()
    return out


def measure(name, cfg, reps, reps_today, dev):
    ev, N = device_stream(cfg, dev)
    E = ev[0].numel()
    g = device_graph(ev, N, dev)
    rows = []
    for what, (nodes, eids) in erasures(ev, N).items():
        def without():
            return g.without(nodes=nodes, eids=eids)._dev
        got = without()
        kept = got[1].numel()
        t_cut = float(ev[2][min(E - 1, E - kept // 2)]) if kept else float('inf')   # keeps about kept / 2 events

        def trimmed():
            return g.trimmed(before=t_cut)._dev
        for _ in range(5):
            got, trm = without(), trimmed()
        torch.cuda.synchronize()
        t = dict(without=[], trimmed=[], today=[])
        for _ in range(reps):   # alternating, every call between its own events
            t['without'].append(timed(without)[0])
            t['trimmed'].append(timed(trimmed)[0])
        ref = None
        for _ in range(reps_today):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = today(ev, N, nodes, eids, dev)
            t['today'].append((time.perf_counter() - t0) * 1e6)
        if ref is not None:
            for a, b in zip(got, ref):
                assert torch.equal(a, b), 'without differs from the build over the filtered events'
        row = dict(shape=name, erasure=what, events=E, nodes=N, reps=reps, reps_today=reps_today, entries=2 * E,
                   entries_kept=kept, entries_kept_by_trim=trm[1].numel(), bit_equal_to_today=ref is not None,
                   ids_marked=int((nodes if nodes is not None else eids).numel()))
        for k in ('without', 'trimmed', 'today'):
            if t[k]:
                row[f'{k}_call_us'] = round(statistics.median(t[k]), 2)
                row[f'{k}_call_us_p10_p90'] = [round(pct(t[k], 0.1), 2), round(pct(t[k], 0.9), 2)]
        per_old = (4 if nodes is not None else 0) + (4 if eids is not None else 0)
        row['without_bytes'] = 2 * E * per_old + 2 * E // 4 + 32 * kept + 24 * N
        row['without_effective_GBps'] = round(row['without_bytes'] / row['without_call_us'] / 1e3, 1)
        row['without_fraction_of_8TBps'] = round(row['without_effective_GBps'] / 8000.0, 4)
        row['without_over_trimmed'] = round(row['without_call_us'] / row['trimmed_call_us'], 2)
        if t['today']:
            row['today_over_without'] = round(row['today_call_us'] / row['without_call_us'], 1)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='c2,c3,big')
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--reps_today', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    rows = []
    for sname in [x for x in a.shapes.split(',') if x]:
        rows += measure(sname, SHAPES[sname], a.reps, a.reps_today, dev)
    out = dict(tool='tcsr_erase_bench', device=torch.cuda.get_device_name(0), results=rows)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
