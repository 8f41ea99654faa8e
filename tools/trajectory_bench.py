#!/usr/bin/env python3
"""Trajectory-encoding measurements (one JSON line, also written to profiles/trajectory_bench_v1.json): C2-shaped
synthetic streams (the stream, model and loader of tools/loop_bench.py --eval) at bs 200 and 1024 - per batch the
resident eval_edge_prediction pass over the same events (the forward encode_trajectory shares; whole call with its
AP / AUC), encode_trajectory as a whole call (numpy table), the pass without the final read-back (as_tensor=True, stream
drained) and the read-back of the [n_nodes, d] float64 table alone.  Everything is timed with HIP events after warm-up;
every sample is kept (median, min, max).

    python tools/trajectory_bench.py [--steps K] [--reps R] [--agg mean] [--out profiles/trajectory_bench_v1.json]
    python tools/trajectory_bench.py --profile-pass 200    # one resident pass at that bs (for rocprofv3 --kernel-trace --stats)
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
from www2023tiger_amd.data.data_loader import BatchLoader, GraphCollator, InteractionData  # noqa: E402
from www2023tiger_amd.eval_utils import encode_trajectory, eval_edge_prediction  # noqa: E402


def samples(fn, reps, warm=2, before=None):
    """ms of fn() over `reps` runs between HIP events (before(): untimed set-up of each run)"""
    out = []
    for r in range(warm + reps):
        if before:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= warm:
            out.append(a.elapsed_time(b))
    return out


def setup(bs, steps):
    c = bench.C2
    E = max((steps + 12) * c['B'], steps * bs)
    st = bench.make_stream(c['n_u'], c['n_i'], E, c['T'] * E / c['E'], seed=0, d_e=c['d'])
    model, _ = bench.build_models(st, c['d'], c['K'], c['msg_src'], c['upd_src'], restarter='static', hist_len=20, dropout=0.1)
    model.eval()
    coll = GraphCollator(model.graph, c['K'], 1, restarter='static', hist_len=20)
    n = steps * bs
    rs = np.random.RandomState(1)
    ev = InteractionData(st['src'][:n], st['dst'][:n], st['ts'][:n], st['eids'][:n], np.zeros(n, dtype=np.int64), seed=0,
                         eval=True, neg_dst=rs.randint(c['n_u'] + 1, c['n_u'] + c['n_i'] + 1, n))
    return model, BatchLoader(ev, bs, coll)


def per_batch(ms, steps):
    us = [x / steps * 1e3 for x in ms]
    return dict(median_us=round(statistics.median(us), 2), min_us=round(min(us), 2), max_us=round(max(us), 2))


def measure(bs, steps, reps, agg):
    model, dl = setup(bs, steps)
    dev = model.device
    out = dict(batches=steps, n_nodes=int(model.n_nodes), d=int(model.nfeat_dim))
    out['eval_edge_prediction_call'] = per_batch(samples(lambda: eval_edge_prediction(model, dl, dev, restart_mode=False),
                                                         reps, before=model.reset), steps)
    out['encode_trajectory_call'] = per_batch(samples(lambda: encode_trajectory(model, dl, dev, agg), reps), steps)
    keep = []

    def on_device():
        keep[:] = [encode_trajectory(model, dl, dev, agg, as_tensor=True)]
        torch.cuda.synchronize()

    out['encode_trajectory_pass_no_readback'] = per_batch(samples(on_device, reps), steps)
    rb = samples(lambda: keep[0].cpu().numpy(), reps)
    out['readback_ms'] = dict(median=round(statistics.median(rb), 3), min=round(min(rb), 3), max=round(max(rb), 3),
                              bytes=int(keep[0].numel() * 8))
    out['extra_us_per_batch_over_eval_call'] = round(out['encode_trajectory_pass_no_readback']['median_us'] -
                                                     out['eval_edge_prediction_call']['median_us'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=500, help='batches per pass')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--agg', default='mean')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'trajectory_bench_v1.json'))
    ap.add_argument('--profile-pass', type=int, default=0, metavar='BS', help='one resident pass at this bs only (for rocprofv3)')
    a = ap.parse_args()
    if a.profile_pass:
        model, dl = setup(a.profile_pass, a.steps)
        encode_trajectory(model, dl, model.device, a.agg, as_tensor=True)  # (first use: one-time set-up)
        t = encode_trajectory(model, dl, model.device, a.agg, as_tensor=True)
        torch.cuda.synchronize()
        print(json.dumps(dict(profile_pass=f'C2 resident bs {a.profile_pass}', batches=a.steps, seen=int(t.any(1).sum()))))
        return
    out = dict(device=torch.cuda.get_device_name(0), agg=a.agg, reps=a.reps)
    for bs in (200, 1024):
        out[f'C2_d172_B{bs}'] = measure(bs, a.steps, a.reps, a.agg)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
