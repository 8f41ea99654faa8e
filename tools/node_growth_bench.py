#!/usr/bin/env python3
"""Node-growth measurements at the C2 shape (one JSON line per run): what admitting new node ids costs the T-CSR extension,
and that the extension WITHOUT growth costs what it did.

    append      tg_tcsr_append of one C2 batch (200 events) onto the C2 graph at 90 % of the stream (141 726 events, 9 228
                nodes) - the entry every commit has, so the same command on a checkout of the parent commit gives the
                parent's figure (--root DIR imports the package of that checkout)
    grow        tg_tcsr_append_grow of the same batch with 6 of its 200 events (3 %) re-pointed at 6 ids nobody has seen:
                every call admits new ids.  Compared bit for bit with tg_tcsr_build_device over all events with the larger
                count.  Skipped (null) where the library lacks the entry.
    grow_nodes  TIGE.grow_nodes(n + 1, reserve=n + 1) on a C2 model (d = 172, sequence restarter), host clock around a
                device synchronise: every call reallocates and copies the two memories, the mailbox and the node table.

Every timed call lies between its own pair of device events after warm-up; a run is `--reps` calls, its figure their median
(with the 10th / 90th percentile), and `queued_us` the time per call of the same number of calls enqueued back to back.  A
process makes `--runs` runs; the spread of a case is max - min over the medians of its runs, in this process - compare it
with the spread between processes by running the tool again.

    python tools/node_growth_bench.py [--root DIR] [--reps 200] [--runs 5] [--no-grow-nodes] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

C2 = dict(n_u=8227, n_i=1000, E=157474, T=2.68e6)
BATCH, NEW_IDS = 200, 6


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def out_arrays(N, P, dev):
    return (torch.empty(N + 1, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.float64, device=dev),
            torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev))


def timed_runs(fn, reps, runs):
    rows = []
    for _ in range(runs):
        t = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1e3)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        rows.append(dict(call_us=round(statistics.median(t), 2), call_us_p10_p90=[round(pct(t, 0.1), 2), round(pct(t, 0.9), 2)],
                         queued_us=round(a.elapsed_time(b) * 1e3 / reps, 2)))
    med = [r['call_us'] for r in rows]
    que = [r['queued_us'] for r in rows]
    return dict(runs=rows, call_us=round(statistics.median(med), 2), call_us_spread=round(max(med) - min(med), 2),
                queued_us=round(statistics.median(que), 2), queued_us_spread=round(max(que) - min(que), 2))


def measure_append(bench, _lib, hip_ops, reps, runs, dev):
    lib, ptr, check, TgTcsr = _lib.lib, _lib.ptr, _lib.check, _lib.TgTcsr
    st = bench.make_stream(C2['n_u'], C2['n_i'], C2['E'], C2['T'], seed=0, with_efeats=False)
    N, E0, n = st['n_nodes'], int(0.9 * C2['E']), BATCH
    ev = tuple(torch.from_numpy(st[k]).to(dev) for k in ('src', 'dst', 'ts', 'eids'))
    s = hip_ops.stream_ptr(dev)
    old, new = tuple(a[:E0] for a in ev), tuple(a[E0:E0 + n].contiguous() for a in ev)
    parent = out_arrays(N, 2 * E0, dev)
    bw = int(lib.tg_tcsr_build_device_workspace_bytes(E0 + n, N + NEW_IDS))
    ws_b = torch.empty(max(bw, 16), dtype=torch.uint8, device=dev)
    check(lib.tg_tcsr_build_device(E0, *(ptr(a) for a in old), N, *(ptr(a) for a in parent), ptr(ws_b), bw, s), 'build')
    g = TgTcsr(N, 2 * E0, *(ptr(a) for a in parent))
    aw = int(lib.tg_tcsr_append_workspace_bytes(2 * E0, n, N))
    ws_a = torch.empty(max(aw, 16), dtype=torch.uint8, device=dev)

    def rebuilt(batch, nodes):
        want = out_arrays(nodes, 2 * (E0 + n), dev)
        both = tuple(torch.cat([a, b]) for a, b in zip(old, batch))
        check(lib.tg_tcsr_build_device(E0 + n, *(ptr(a) for a in both), nodes, *(ptr(a) for a in want), ptr(ws_b), bw, s), 'rebuild')
        torch.cuda.synchronize()
        return want
    got = out_arrays(N, 2 * (E0 + n), dev)

    def append():
        check(lib.tg_tcsr_append(C.byref(g), n, *(ptr(a) for a in new), *(ptr(a) for a in got), ptr(ws_a), aw, s), 'append')
    for _ in range(20):
        append()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, rebuilt(new, N))), 'the extension differs from the rebuild'
    out = dict(shape='c2', events_old=E0, events_new=n, nodes=N, reps=reps, append=timed_runs(append, reps, runs), grow=None)
    if hasattr(lib, 'tg_tcsr_append_grow'):   # (a checkout of the parent commit lacks the entry)
        N1 = N + NEW_IDS
        src = new[0].clone()
        src[torch.linspace(0, n - 1, NEW_IDS, device=dev).long()] = torch.arange(N, N1, device=dev)
        batch = (src,) + new[1:]
        got1 = out_arrays(N1, 2 * (E0 + n), dev)

        def grow():
            check(lib.tg_tcsr_append_grow(C.byref(g), N1, n, *(ptr(a) for a in batch), *(ptr(a) for a in got1), ptr(ws_a), aw, s),
                  'append_grow')
        for _ in range(20):
            grow()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got1, rebuilt(batch, N1))), 'the growing extension differs from the rebuild'
        out['grow'] = dict(timed_runs(grow, reps, runs), nodes_out=N1, new_ids_per_call=NEW_IDS)
    return out


def measure_grow_nodes(bench, dev, calls=7):
    st = bench.make_stream(C2['n_u'], C2['n_i'], C2['E'], C2['T'], seed=0, d_e=172)
    model, _ = bench.build_models(st, d=172, K=10, msg_src='left', upd_src='right', restarter='seq', device=str(dev))
    if not hasattr(model, 'grow_nodes'):
        return None
    model.eval()
    t = []
    for i in range(calls):
        n = model.n_nodes + 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        moved = model.grow_nodes(n, reserve=n)   # a store without head-room: the next call reallocates too
        torch.cuda.synchronize()
        assert moved
        if i >= 2:
            t.append((time.perf_counter() - t0) * 1e6)
    d = model.memory_dim
    nbytes = model.n_nodes * (2 * (4 * d + 5) + 4 * model.raw_msg_dim + 4 + 4 * d)
    return dict(nodes=st['n_nodes'], d=d, calls=len(t), reallocating_call_us=round(statistics.median(t), 1),
                reallocating_call_us_min_max=[round(min(t), 1), round(max(t), 1)], table_bytes=nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='the checkout whose package and bench.py are measured (default: this one)')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--no-grow-nodes', action='store_true')
    ap.add_argument('--label', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import bench
    from www2023tiger_amd import _lib, hip_ops
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(a.root)), _lib.__file__
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    out = dict(tool='node_growth_bench', label=a.label, device=torch.cuda.get_device_name(0),
               tcsr=measure_append(bench, _lib, hip_ops, a.reps, a.runs, dev))
    out['grow_nodes'] = None if a.no_grow_nodes else measure_grow_nodes(bench, dev)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
