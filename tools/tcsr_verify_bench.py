#!/usr/bin/env python3
"""T-CSR verifier measurements (one JSON line).

Per shape, on one device-resident graph (the parents of tools/tcsr_append_bench.py: the first 90 % of the stream), three
ways to answer "may the library read these four arrays?" - the six classes and the maximum time of tg_tcsr_verify:

    verify    `hip_ops.tcsr_verify(graph, eid_rows)`: three launches (tiles of 2048 entries, the row bounds, one fold) and
              ONE read-back of the 8 result words (tg_verify.hip);
    torch     the same six checks and the maximum written with torch reductions on the device and one read-back of the
              stacked results - what a caller has without the kernel (row starts: a scatter of indptr into a flag array,
              which is only legal once indptr itself has been checked);
    host      download the four arrays and run the host twin (`hip_ops.tcsr_verify_host`).

`verify` and `torch` alternate for `reps` repetitions after warm-up, each call between its own pair of device events
(median, 10th / 90th percentile; both contain one read-back).  `host` is timed with a host clock around a device
synchronise, `reps_host` times.  The three results are compared (all clean, the same maximum).  The effective rate is the
bytes a verification must read - 20 per entry (time, neighbour, eid; the time in front comes from the cache), 8 per node -
over the median call time.  Shapes:

    c2    141 726 events of the C2 stream (bench.make_stream: 9 228 nodes)
    c3    605 202 events of the C3 stream (10 985 nodes)
    big   9 000 000 events over 1 M nodes, generated on the device (beyond the last-level cache)

Only `big` says anything about HBM bandwidth (peak 8 TB/s); c2 and c3 fit the caches and are bound by their launches and
the read-back.  Then the wall time of `TIGE.save_online` (to a file in a temporary directory) and `TIGE.load_online` (into
a second model built on a stub graph) of a C2 model (d = 172) that has streamed its stream.

    python tools/tcsr_verify_bench.py [--shapes c2,c3,big] [--reps 100] [--reps_host 3] [--no-model] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcsr_append_bench import SHAPES, device_stream, pct  # noqa: E402
from tcsr_trim_bench import device_graph, timed  # noqa: E402
from www2023tiger_amd import hip_ops  # noqa: E402


def torch_verify(arrays, N, rows):
    """the six classes and the maximum with torch reductions -> (code, first[6], t_max); one read-back"""
    indptr, ts, nbr, eid = arrays
    P = ts.numel()
    dev = ts.device
    big = torch.iinfo(torch.int64).max
    first = lambda mask, base=0: (torch.where(mask, torch.arange(base, base + mask.numel(), device=dev), big).min()
                                  if mask.numel() else torch.tensor(big, device=dev))
    ends = torch.where(indptr[0] != 0, 0, torch.where(indptr[N] != P, N, big))
    ptr_order = first(indptr[1:] < indptr[:-1])
    nan = ts != ts
    start = torch.zeros(P + 1, dtype=torch.bool, device=dev)
    start[indptr.clamp(0, P)] = True   # (the loaded values index the flags: legal only because they are clamped here)
    ts_order = first((ts[1:] < ts[:-1]) & ~start[1:P], 1) if P > 1 else torch.tensor(big, device=dev)
    res = torch.stack([ends, ptr_order, ts_order, first(nan), first((nbr < 0) | (nbr >= N)),
                       first((eid & 0x7FFFFFFF) >= rows) if rows >= 0 else torch.tensor(big, device=dev)])
    t_max = torch.where(nan, -float('inf'), ts).max() if P else torch.tensor(-float('inf'), dtype=torch.float64, device=dev)
    out = torch.cat([res.double(), t_max.reshape(1)]).tolist()   # (indices are exact in float64 below 2^53; big is not one)
    f = [-1 if x >= 2.0 ** 62 else int(x) for x in out[:6]]
    if f[0] >= 0 or f[1] >= 0:
        f[2] = -1
    return sum(1 << c for c in range(6) if f[c] >= 0), f, out[6]


def measure(name, cfg, reps, reps_host, dev):
    ev, N = device_stream(cfg, dev)
    E = int(0.9 * ev[0].numel())
    ev = tuple(a[:E].contiguous() for a in ev)
    g = device_graph(ev, N, dev)
    rows = E + 1

    def verify():
        return hip_ops.tcsr_verify(g, rows)

    def by_torch():
        return torch_verify(g._dev, N, rows)
    for _ in range(5):
        got, ref = verify(), by_torch()
    assert got == ref and got[0] == 0, (got, ref)
    torch.cuda.synchronize()
    t = dict(verify=[], torch=[], host=[])
    for _ in range(reps):   # alternating, every call between its own events
        t['verify'].append(timed(verify)[0])
        t['torch'].append(timed(by_torch)[0])
    for _ in range(reps_host):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = hip_ops.tcsr_verify_host(tuple(a.cpu().numpy() for a in g._dev), rows)
        t['host'].append((time.perf_counter() - t0) * 1e6)
        assert host == got
    row = dict(shape=name, events=E, nodes=N, entries=2 * E, reps=reps, reps_host=reps_host, results_equal=True)
    for k in ('verify', 'torch', 'host'):
        if t[k]:
            row[f'{k}_call_us'] = round(statistics.median(t[k]), 2)
            row[f'{k}_call_us_p10_p90'] = [round(pct(t[k], 0.1), 2), round(pct(t[k], 0.9), 2)]
    row['verify_bytes'] = 20 * 2 * E + 8 * N
    row['verify_effective_GBps'] = round(row['verify_bytes'] / row['verify_call_us'] / 1e3, 1)
    row['verify_fraction_of_8TBps'] = round(row['verify_effective_GBps'] / 8000.0, 4)
    row['torch_over_verify'] = round(row['torch_call_us'] / row['verify_call_us'], 2)
    if t['host']:
        row['host_over_verify'] = round(row['host_call_us'] / row['verify_call_us'], 1)
    return row


def model_round_trip(dev, reps=3):
    """save_online / load_online wall time of a C2 model that has streamed its stream"""
    import bench
    c = bench.C2
    st = bench.make_stream(c['n_u'], c['n_i'], c['E'], c['T'], seed=0, d_e=c['d'])
    kw = dict(d=c['d'], K=c['K'], msg_src=c['msg_src'], upd_src=c['upd_src'], restarter='seq', dropout=0.0, device=str(dev))
    model, _ = bench.build_models(st, **kw)
    B = c['B']
    for lo in range(0, 20 * B, B):
        model.stream_step(*(st[k][lo:lo + B] for k in ('src', 'dst', 'neg', 'ts', 'eids')))
    stub = {k: (v[:3] if k in ('src', 'dst', 'neg', 'ts', 'eids') else v) for k, v in st.items()}
    stub['efeats'] = st['efeats'][:4]
    other, _ = bench.build_models(stub, seed=1, **kw)
    t_save, t_load, size = [], [], 0
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'served.pt')
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.save_online(path)
            t_save.append(time.perf_counter() - t0)
            size = os.path.getsize(path)
            t0 = time.perf_counter()
            other.load_online(path)
            torch.cuda.synchronize()
            t_load.append(time.perf_counter() - t0)
    for a, b in zip(model.graph._tensors(), other.graph._tensors()):
        assert torch.equal(a, b)
    assert torch.equal(model.left_memory.vals, other.left_memory.vals)
    return dict(shape='c2 model', d=c['d'], nodes=st['n_nodes'], events=c['E'], edge_table_rows=c['E'] + 1, reps=reps,
                file_MB=round(size / 1e6, 1), save_online_ms=round(statistics.median(t_save) * 1e3, 1),
                load_online_ms=round(statistics.median(t_load) * 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='c2,c3,big')
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--reps_host', type=int, default=3)
    ap.add_argument('--no-model', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    rows = [measure(s, SHAPES[s], a.reps, a.reps_host, dev) for s in a.shapes.split(',') if s]
    out = dict(tool='tcsr_verify_bench', device=torch.cuda.get_device_name(0), results=rows)
    if not a.no_model:
        out['model_round_trip'] = model_round_trip(dev)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
