#!/usr/bin/env python3
"""Ranking-evaluation measurements (one JSON line, also written to profiles/rank_eval_bench_v1.json): the C2-shaped
synthetic stream (d = 172, K = 10) at B = 200 events with C = 20 and C = 100 random candidate destinations per event.

Per batch, on a state warmed by `--warm` streamed batches:
  rank_scores      TIGE.rank_scores: the B (2 + C) embeddings on the operator path + tg_rank_scores (whole call)
  score_head       tg_rank_scores alone, on operands of the same shapes (its flop count 2 B (1 + C) W d against the
                   157.3 TF/s float32 MFMA peak); embedding = rank_scores - score_head
  step_per_column  the only way to these scores through the public API WITHOUT rank_scores: C calls of the one-call
                   evaluation step (contrast_learning under no_grad) with neg = cand[:, j], each on a restored
                   save_memory_state() snapshot
Both are timed in this run on this device with HIP events after warm-up, alternating, `--reps` samples each (median, min,
max kept); the largest difference between the two score matrices of one batch is reported beside them.

    python tools/rank_eval_bench.py [--steps K] [--reps R] [--out profiles/rank_eval_bench_v1.json]
    python tools/rank_eval_bench.py --profile-pass 100    # rank_scores only, C = 100 (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from www2023tiger_amd._lib import check, lib, ptr  # noqa: E402
from www2023tiger_amd.data.data_loader import GraphCollator  # noqa: E402
from www2023tiger_amd.hip_ops import stream_ptr  # noqa: E402
from www2023tiger_amd.model.training import score_struct  # noqa: E402

PEAK_F32_MFMA = 157.3e12
B = 200


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms, per):
    v = [x / per for x in ms]
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def setup(warm, steps):
    c = bench.C2
    E = (warm + steps) * B
    st = bench.make_stream(c['n_u'], c['n_i'], E, c['T'] * E / c['E'], seed=0, d_e=c['d'])
    model, _ = bench.build_models(st, c['d'], c['K'], c['msg_src'], c['upd_src'], restarter='static', hist_len=20, dropout=0.1)
    model.eval()
    for b in range(warm):
        model.stream_step(*[st[k][b * B:(b + 1) * B] for k in ('src', 'dst', 'neg', 'ts', 'eids')])
    dev = model.device
    t = lambda k, dt: torch.as_tensor(st[k][warm * B:]).to(dev, dt)
    cols = dict(src=t('src', torch.int64), dst=t('dst', torch.int64), ts=t('ts', torch.float64), eids=t('eids', torch.int64))
    return model, st, cols


def batches(cols, steps):
    for b in range(steps):
        sl = slice(b * B, (b + 1) * B)
        yield cols['src'][sl], cols['dst'][sl], cols['ts'][sl], cols['eids'][sl]


def step_per_column(model, coll, snap, src, dst, ts, eids, cand):
    """C evaluation steps, each on the restored snapshot -> scores [B, 1 + C]"""
    out = torch.empty(len(src), cand.shape[1] + 1, device=src.device)
    for j in range(cand.shape[1]):
        model.load_memory_state(tuple(x.clone() for x in snap))
        neg = cand[:, j].contiguous()
        a = coll.collate_tensors(src, dst, neg, ts, eids)
        _, _, pos, ns, *_ = model.contrast_learning(a[0], a[1], a[2], a[3], a[4], a[6])
        out[:, 1 + j] = ns
        out[:, 0] = pos
    model.load_memory_state(tuple(x.clone() for x in snap))
    return out


def score_head_alone(model, Cn, reps, inner=20):
    d, K, dev = model.memory_dim, model.n_neighbors, model.device
    g = torch.Generator(device='cpu').manual_seed(0)
    h_src = torch.randn(B, d, generator=g).to(dev)
    h_cand = torch.randn(B * (Cn + 1), d, generator=g).to(dev)
    ids = lambda *s: torch.randint(0, model.n_nodes, s, generator=g).to(dev)
    nb_src, nb_cand, src, cand = ids(B, K), ids(B * (Cn + 1), K), ids(B), ids(B, Cn + 1)
    sp = score_struct(model)
    ws = torch.empty(int(lib.tg_rank_scores_workspace_bytes(B, d, C.byref(sp))), dtype=torch.uint8, device=dev)
    out = torch.empty(B, Cn + 1, device=dev)

    def run():
        for _ in range(inner):
            check(lib.tg_rank_scores(B, Cn, d, K, C.byref(sp), ptr(h_src), ptr(h_cand), ptr(nb_src), ptr(nb_cand), ptr(src),
                                     ptr(cand), ptr(out), ptr(ws), ws.numel(), stream_ptr(dev)), 'tg_rank_scores')

    run()
    return stats([timed(run) for _ in range(reps)], inner)


def measure(model, st, cols, Cn, steps, reps):
    c = bench.C2
    dev = model.device
    coll = GraphCollator(model.graph, c['K'], 1, restarter='static', hist_len=20)
    rs = np.random.RandomState(7)
    cand = torch.from_numpy(rs.randint(c['n_u'] + 1, c['n_u'] + c['n_i'] + 1, (steps * B, Cn))).to(dev)
    snap = model.save_memory_state()
    bl = list(batches(cols, steps))
    ours = lambda: [model.rank_scores(s, d_, t, cand[i * B:(i + 1) * B]) for i, (s, d_, t, _) in enumerate(bl)]
    theirs = lambda: [step_per_column(model, coll, snap, s, d_, t, e, cand[i * B:(i + 1) * B])
                      for i, (s, d_, t, e) in enumerate(bl)]
    a, b = ours(), theirs()  # warm-up of every shape, and the agreement of the two
    diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
    t_ours, t_theirs = [], []
    for _ in range(reps):  # alternating
        t_ours.append(timed(ours))
        t_theirs.append(timed(theirs))
    d, W = model.memory_dim, model.memory_dim
    out = dict(C=Cn, batches=steps, pairs_per_batch=B * (Cn + 1), queries_per_batch=B * (Cn + 2),
               rank_scores=stats(t_ours, steps), step_per_column=stats(t_theirs, steps),
               score_head=score_head_alone(model, Cn, reps), max_abs_score_diff=diff)
    ms = out['rank_scores']['median_ms']
    out['pairs_per_s'] = round(B * (Cn + 1) / (ms * 1e-3))
    out['embedding_ms'] = round(ms - out['score_head']['median_ms'], 4)
    flops = 2.0 * B * (Cn + 1) * W * d
    out['score_head_flops'] = flops
    out['score_head_fraction_of_f32_mfma_peak'] = round(flops / (out['score_head']['median_ms'] * 1e-3) / PEAK_F32_MFMA, 5)
    out['speedup_over_step_per_column'] = round(out['step_per_column']['median_ms'] / ms, 2)
    return out


def clocks():
    """what the runtime reports about the device and its clocks; a field this torch build does not have is left out"""
    p = torch.cuda.get_device_properties(0)
    out = dict(device=p.name, compute_units=p.multi_processor_count)
    for name, attr in (('max_engine_clock_mhz', 'clock_rate'), ('max_memory_clock_mhz', 'memory_clock_rate')):
        v = getattr(p, attr, None)
        if v is not None:
            out[name] = v / 1e3
    try:
        out['engine_clock_now_mhz'] = torch.cuda.clock_rate()
    except Exception as e:  # the management library is optional
        out['engine_clock_now_mhz'] = f'unavailable ({type(e).__name__})'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=4, help='timed batches per sample')
    ap.add_argument('--warm', type=int, default=40, help='streamed batches before the measurement')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rank_eval_bench_v1.json'))
    ap.add_argument('--profile-pass', type=int, default=0, metavar='C', help='rank_scores only, at this C (for rocprofv3)')
    a = ap.parse_args()
    model, st, cols = setup(a.warm, a.steps)
    if a.profile_pass:
        c = bench.C2
        cand = torch.from_numpy(np.random.RandomState(7).randint(c['n_u'] + 1, c['n_u'] + c['n_i'] + 1, (B, a.profile_pass))).to(model.device)
        for s, d_, t, _ in list(batches(cols, a.steps)) * 2:
            model.rank_scores(s, d_, t, cand)
        torch.cuda.synchronize()
        print(json.dumps(dict(profile_pass=f'C2 rank_scores B {B} C {a.profile_pass}', calls=2 * a.steps)))
        return
    out = dict(workload='C2-shaped stream, d 172, K 10, B 200, rnd candidates', reps=a.reps, warm_batches=a.warm, clocks=clocks())
    for Cn in (20, 100):
        out[f'C{Cn}'] = measure(model, st, cols, Cn, a.steps, a.reps)
    out['clocks_after'] = clocks().get('engine_clock_now_mhz')
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
