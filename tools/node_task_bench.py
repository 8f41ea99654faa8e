#!/usr/bin/env python3
"""Node-classification measurements (one JSON line): the evaluation pass of eval_node_classification in events/s at
C1 (d = 172, B = 100: the reference's node-task batch) and C2 (B = 1024) shapes, resident stream against the
per-batch loop (TG_EVAL_RESIDENT=0), with the link-prediction pass over the same events for the decoder's share; the
decoder's training iteration (forward + BCE + backward + Adam) on the fused kernels against the same nn.Sequential on
plain torch; tg_roc_auc at n = 1e5 and 2^22.  Everything is timed with HIP events after warm-up.

    python tools/node_task_bench.py [--events N] [--reps R]
    python tools/node_task_bench.py --profile-pass      # one resident C1 pass (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from www2023tiger_amd._lib import lib, ptr  # noqa: E402
from www2023tiger_amd.data.data_loader import BatchLoader, GraphCollator, InteractionData  # noqa: E402
from www2023tiger_amd.eval_utils import eval_edge_prediction, eval_node_classification  # noqa: E402
from www2023tiger_amd.hip_ops import stream_ptr  # noqa: E402
from www2023tiger_amd.model.basic_modules import MLP  # noqa: E402
from www2023tiger_amd.optim import Adam  # noqa: E402


def timed(fn, reps, warm=1, before=None):
    """median ms of fn() over `reps` runs between HIP events (before(): untimed set-up of each run)"""
    for _ in range(warm):
        if before:
            before()
        fn()
    out = []
    for _ in range(reps):
        if before:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def setup(cfg, B, n_events):
    st = bench.make_stream(cfg['n_u'], cfg['n_i'], max(cfg['E'], n_events), cfg['T'], seed=0, d_e=cfg['d'])
    model, _ = bench.build_models(st, cfg['d'], cfg['K'], cfg['msg_src'], cfg['upd_src'], restarter='static', dropout=0.1)
    model.eval()
    coll = GraphCollator(model.graph, cfg['K'], 1, restarter='static')
    labels = (np.random.RandomState(1).uniform(size=n_events) < 0.1).astype(np.int64)
    data = InteractionData(st['src'][:n_events], st['dst'][:n_events], st['ts'][:n_events], st['eids'][:n_events], labels,
                           seed=0, eval=True)
    torch.manual_seed(0)
    decoder = MLP(cfg['d'], dropout=0.1).to(model.device)
    return model, decoder, BatchLoader(data, B, coll)


def eval_rates(cfg, B, n_events, reps):
    model, decoder, dl = setup(cfg, B, n_events)
    out = {}
    for name, env in (('resident', '1'), ('loop', '0')):
        os.environ['TG_EVAL_RESIDENT'] = env
        ms = timed(lambda: eval_node_classification(model, decoder, dl, model.device), reps, before=model.reset)
        out[f'node_{name}_events_per_s'] = round(n_events / ms * 1e3)
    os.environ['TG_EVAL_RESIDENT'] = '1'
    ms = timed(lambda: eval_edge_prediction(model, dl, model.device, restart_mode=False), reps, before=model.reset)
    out['edge_resident_events_per_s'] = round(n_events / ms * 1e3)
    out['decoder_share_us_per_batch'] = round((n_events / out['node_resident_events_per_s'] -
                                               n_events / out['edge_resident_events_per_s']) / (n_events / B) * 1e6, 2)
    return out


def train_iter_us(d, B, iters=200):
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    x, y = torch.randn(B, d, device=dev), (torch.rand(B, device=dev) < 0.3).float()
    loss_fn = nn.BCEWithLogitsLoss()
    fused = MLP(d, dropout=0.1).to(dev).train()
    plain = nn.Sequential(nn.Linear(d, 80), nn.ReLU(), nn.Dropout(0.1), nn.Linear(80, 10), nn.ReLU(), nn.Dropout(0.1),
                          nn.Linear(10, 1)).to(dev).train()
    res = {}
    for name, mod, opt in (('fused', fused, Adam(fused.parameters(), lr=3e-4)),
                           ('torch', plain, torch.optim.Adam(plain.parameters(), lr=3e-4))):
        def it():
            for _ in range(iters):
                opt.zero_grad()
                loss_fn(mod(x).squeeze(-1), y).backward()
                opt.step()
        res[name] = round(timed(it, 3) / iters * 1e3, 2)
    return res


def auc_ms(n, reps=20):
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    s = torch.rand(n, device=dev, generator=g)
    lab = (torch.rand(n, device=dev, generator=g) < 0.3).float()
    ws = torch.empty(int(lib.tg_roc_auc_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    auc = torch.empty(1, dtype=torch.float64, device=dev)

    def call():
        lib.tg_roc_auc(n, ptr(s), ptr(lab), ptr(auc), None, ptr(ws), ws.numel(), stream_ptr(dev))
    call()
    return round(timed(lambda: [call() for _ in range(reps)], 3) / reps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--events', type=int, default=20000, help='events per evaluation pass')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--profile-pass', action='store_true', help='one resident C1 pass only (for rocprofv3)')
    a = ap.parse_args()
    c1 = dict(bench.WORKLOADS['c1'], B=100)
    if a.profile_pass:
        model, decoder, dl = setup(c1, 100, a.events)
        model.reset()
        eval_node_classification(model, decoder, dl, model.device)  # (first use: one-time set-up)
        model.reset()
        auc = eval_node_classification(model, decoder, dl, model.device)
        torch.cuda.synchronize()
        print(json.dumps(dict(profile_pass='C1 resident', events=a.events, auc=auc)))
        return
    out = dict(device=torch.cuda.get_device_name(0), events=a.events)
    out['C1_d172_B100'] = eval_rates(c1, 100, a.events, a.reps)
    out['C2_d172_B1024'] = eval_rates(bench.C2, 1024, a.events, a.reps)
    out['decoder_train_iter_us'] = {'d172_B100': train_iter_us(172, 100), 'd172_B1024': train_iter_us(172, 1024)}
    out['roc_auc_ms'] = {'n_1e5': auc_ms(100000), 'n_2^22': auc_ms(1 << 22)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
