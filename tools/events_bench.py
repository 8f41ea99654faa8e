#!/usr/bin/env python3
"""Event-key measurements (one JSON line).

Per (batch B, share of duplicates p) - B = 1 024 and 65 536 delivered events, p = 0 %, 10 %, 100 % of them redeliveries (half
copies of events the tracker holds, half copies inside the batch; at 100 % all are copies of held events):

  the kernel yardstick
    screen_commit   `EventKeys.screen(keys)` + `EventKeys.commit(keys[keep])` on a tracker of --rows rows: tg_events_screen (one
                    launch for n <= 256, five above; one read-back) and tg_idmap_assign over the kept keys (one read-back);
    assign          `IdMap.assign` of the SAME n keys on a map that holds the same keys: what the library already pays to
                    turn a batch of keys into numbers.
    Every repetition starts from the same tables (copied back outside the timed region).
  the end-to-end overhead, both on the same build
    observe_events  `TIGE.observe_events` of the delivered batch on a tracked model;
    observe         `TIGE.observe` of the same CLEAN batch (the (1 - p) B new events) on a twin with equal weights.
    Both models walk the same stream (bench.make_stream, d = 32, K = 10); at p = 100 % nothing is new: `observe` has nothing
    to do and only `observe_events` is timed (it keeps nothing and streams nothing).

Each call between its own pair of device events after warm-up (median, 10th / 90th percentile).

    python tools/events_bench.py [--batches 1024,65536] [--dups 0,0.1,1] [--rows 1000000] [--reps 30] [--e2e_reps 8] [--out FILE]
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
from www2023tiger_amd.data.events import EventKeys  # noqa: E402
from www2023tiger_amd.data.idmap import IdMap  # noqa: E402

MULT = np.uint64(0x9E3779B97F4A7C15)   # odd: distinct integers give distinct keys


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def stats(name, xs):
    return {f'{name}_call_us': round(statistics.median(xs), 2), f'{name}_call_us_p10_p90': [round(pct(xs, 0.1), 2), round(pct(xs, 0.9), 2)]}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, r


def keys_of_range(lo, hi):
    return (np.arange(lo, hi, dtype=np.uint64) * MULT).astype(np.int64)


def delivered(held, n, p, rep):
    """positions of a delivered batch: (1 - p) n new keys in order, p n copies - of held keys and of the batch itself - among
    them -> (keys int64 [n], number of new keys)"""
    rs = np.random.RandomState(1000 + rep)
    n_dup = int(round(p * n))
    fresh = keys_of_range((1 << 40) + rep * n, (1 << 40) + rep * n + n - n_dup)
    n_old = n_dup if fresh.size == 0 else n_dup // 2
    copies = np.concatenate([held[rs.randint(0, len(held), size=n_old)],
                             fresh[rs.randint(0, max(fresh.size, 1), size=n_dup - n_old)] if fresh.size else fresh[:0]])
    keys = np.concatenate([fresh, copies])   # (a copy inside the batch stands behind its original)
    return keys, fresh.size


def kernel_yardstick(rows, n, p, reps, dev):
    held = keys_of_range(1, rows)
    ev = EventKeys(dev, rows, torch.from_numpy(held))
    ev.reserve(n)
    im = IdMap.from_keys(torch.from_numpy(held), dev)
    im._grow(im.size + n)
    pristine = [t.clone() for t in ev.tables + im.tables]
    sc, asg, kept = [], [], 0
    for rep in range(-3, reps):
        keys_np, n_new = delivered(held, n, p, rep + 3)
        keys = torch.from_numpy(keys_np).to(dev)
        for t, src in zip(ev.tables + im.tables, pristine):
            t.copy_(src)
        ev.size = im.size = rows
        im.slots_used = rows

        def screen_commit():
            eids, keep = ev.screen(keys)
            ev.commit(keys[keep])
            return eids, keep
        us_s, (eids, keep) = timed(screen_commit)
        us_a, ids = timed(lambda: im.assign(keys))
        assert keep.numel() == n_new and ev.size == rows + n_new == im.size and torch.equal(eids, ids)   # the same numbers
        kept = n_new
        if rep >= 0:
            sc.append(us_s)
            asg.append(us_a)
    out = dict(rows=rows, batch=n, share_dup=p, kept=kept, reps=reps, launches_screen=1 if n <= 256 else 5, results_checked=True)
    out.update(stats('screen_commit', sc))
    out.update(stats('assign', asg))
    out['screen_commit_over_assign'] = round(out['screen_commit_call_us'] / out['assign_call_us'], 2)
    return out


def end_to_end(n, p, reps, dev):
    import bench
    n_new = n - int(round(p * n))
    warm = 4096
    E = warm + (reps + 2) * max(n_new, 1) + n
    st = bench.make_stream(20000, 2000, E, 1.0e6, seed=0, d_e=32, integer_ts=False, with_efeats=True)
    models = []
    for _ in range(2):
        from www2023tiger_amd.data.graph import Graph
        m, _ = bench.build_models(st, 32, 10, 'left', 'right', dropout=0.0)
        m.graph = Graph.from_arrays(*(st[k][:warm] for k in ('src', 'dst', 'ts', 'eids')), strategy='recent_edges', seed=0,
                                    max_node_id=st['n_nodes'] - 1, device=dev)
        m.raw_feat_getter.efeats = m.raw_feat_getter.efeats[:warm + 1].clone()
        m.invalidate_struct()
        m.stream_step(*[st[k][:warm] for k in ('src', 'dst', 'dst', 'ts', 'eids')])
        models.append(m)
    plain, tracked = models
    all_keys = keys_of_range(1, E + 1)
    key = lambda idx: torch.from_numpy(all_keys[idx])
    tracked.track_events(key(np.arange(warm)))
    ef = torch.from_numpy(st['efeats']).to(dev)
    t_obs, t_ev, lo = [], [], warm
    for rep in range(-2, reps):
        rs = np.random.RandomState(rep + 2)
        cur = np.arange(lo, lo + n_new)
        n_dup = n - n_new
        old = rs.randint(max(lo - n, 0), lo, size=n_dup if n_new == 0 else n_dup // 2)
        inner = cur[rs.randint(0, n_new, size=n_dup - old.size)] if n_new else cur[:0]
        idx = np.concatenate([old, cur, inner])
        a = [torch.from_numpy(st[k][idx]).to(dev) for k in ('src', 'dst', 'ts')]
        k, rows_e = key(idx).to(dev), ef[torch.from_numpy(idx + 1).to(dev)]   # (made outside the timed region)
        us_e, (step, adm) = timed(lambda: tracked.observe_events(*a, k, efeats=rows_e))
        assert adm.n_kept == n_new
        us_o = None
        if n_new:
            c = [torch.from_numpy(st[k][cur]).to(dev) for k in ('src', 'dst', 'ts')]
            rows = plain.raw_feat_getter.efeats.shape[0]
            eids, rows_c = torch.arange(rows, rows + n_new, device=dev), ef[torch.from_numpy(cur + 1).to(dev)]
            us_o, buf = timed(lambda: plain.observe(*c, eids, efeats=rows_c))
            assert torch.equal(buf.h[:2 * n_new], step.h[:2 * n_new])   # the same model
        lo += n_new
        if rep >= 0:
            t_ev.append(us_e)
            if us_o is not None:
                t_obs.append(us_o)
    out = dict(batch=n, share_dup=p, kept=n_new, reps=reps, d=32, n_neighbors=10)
    out.update(stats('observe_events', t_ev))
    if t_obs:
        out.update(stats('observe', t_obs))
        out['observe_events_over_observe'] = round(out['observe_events_call_us'] / out['observe_call_us'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1024,65536')
    ap.add_argument('--dups', default='0,0.1,1')
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--e2e_reps', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    kernels, e2e = [], []
    for n in (int(x) for x in a.batches.split(',')):
        for p in (float(x) for x in a.dups.split(',')):
            kernels.append(kernel_yardstick(a.rows, n, p, a.reps, dev))
            e2e.append(end_to_end(n, p, a.e2e_reps, dev))
    line = json.dumps({'tool': 'events_bench', 'device': torch.cuda.get_device_name(0), 'one_max': 256, 'kernels': kernels,
                       'end_to_end': e2e})
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
