#!/usr/bin/env python3
"""Catalogue-snapshot measurements (one JSON line, also written to profiles/recommend_snapshot_v1.json): the C2-shaped
synthetic stream (d = 172, K = 10, 'bin' hits) on a state warmed by `--warm` streamed batches of 200 events; B users ask
at ONE time for their k = 10 best items of a shared catalogue of C items.

For (B, C) in (200, 1000 = all destinations of the stream), (1, 1000), (200, all 9227 node ids), (1, all node ids):
  recommend_tensors    TIGE.recommend(src, ts, cat, k): B (1 + C) embeddings + tg_rank_scores + tg_topk_rows - the code of
                       the parent commit, so the baseline
  embed_catalogue      TIGE.embed_catalogue(cat, t): C embeddings
  recommend_snapshot   TIGE.recommend(src, ts, snapshot, k) on a ready snapshot whose P is current: B embeddings +
                       tg_rank_scores_shared + tg_topk_rows
  cand_half            tg_rank_cand_half alone (C rows; its flop count 2 C d^2 against the 157.3 TF/s float32 MFMA peak)
  scores_shared        tg_rank_scores_shared alone on operands of the same shapes.  Its pair pass does 6 float32 vector
                       operations per (pair, hidden column) for 'bin' / 'count' - P + S, T_s + T_d, + that sum, max, * w2,
                       + into the partial sum - none of them fused and none of them packed by the source, so 6 B C d
                       operations are set against the 157.3 TFLOP/s vector peak (which counts a packed FMA as 4) and
                       against a quarter of it (the issue rate of unpacked, unfused operations)
All timed in this run on this device with HIP events after a warm-up call, `--reps` samples each (median, min, max kept);
the lists of the two recommend forms are compared exactly before anything is timed.

    python tools/recommend_bench.py [--reps R] [--out profiles/recommend_snapshot_v1.json]
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
from www2023tiger_amd.hip_ops import stream_ptr  # noqa: E402
from www2023tiger_amd.model.training import score_struct  # noqa: E402

PEAK_F32 = 157.3e12   # vector = matrix peak, FLOP/s
BS = 200


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms, per=1):
    v = [x / per for x in ms]
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def setup(warm):
    c = bench.C2
    E = (warm + 2) * BS
    st = bench.make_stream(c['n_u'], c['n_i'], E, c['T'] * E / c['E'], seed=0, d_e=c['d'])
    model, _ = bench.build_models(st, c['d'], c['K'], c['msg_src'], c['upd_src'], restarter='static', hist_len=20, dropout=0.1)
    model.eval()
    for b in range(warm):
        model.stream_step(*[st[k][b * BS:(b + 1) * BS] for k in ('src', 'dst', 'neg', 'ts', 'eids')])
    return model, st


def kernels_alone(model, B, Cn, reps, inner=20):
    d, K, dev = model.memory_dim, model.n_neighbors, model.device
    g = torch.Generator(device='cpu').manual_seed(0)
    h_src, h_cat = torch.randn(B, d, generator=g).to(dev), torch.randn(Cn, d, generator=g).to(dev)
    ids = lambda *s: torch.randint(0, model.n_nodes, s, generator=g).to(dev)
    nb_src, nb_cat, src, cat = ids(B, K), ids(Cn, K), ids(B), ids(Cn)
    sp = score_struct(model)
    P = torch.empty(Cn, d, device=dev)
    ws = torch.empty(int(lib.tg_rank_scores_shared_workspace_bytes(B, d, C.byref(sp))), dtype=torch.uint8, device=dev)
    out = torch.empty(B, Cn, device=dev)

    def half():
        for _ in range(inner):
            check(lib.tg_rank_cand_half(Cn, d, K, C.byref(sp), ptr(h_cat), ptr(P), stream_ptr(dev)), 'tg_rank_cand_half')

    def shared():
        for _ in range(inner):
            check(lib.tg_rank_scores_shared(B, Cn, d, K, C.byref(sp), ptr(h_src), ptr(P), ptr(nb_src), ptr(nb_cat), ptr(src),
                                            ptr(cat), ptr(out), Cn, ptr(ws), ws.numel(), stream_ptr(dev)), 'tg_rank_scores_shared')

    half()
    shared()
    th, tsh = stats([timed(half) for _ in range(reps)], inner), stats([timed(shared) for _ in range(reps)], inner)
    ops = 6.0 * B * Cn * d
    sec = tsh['median_ms'] * 1e-3
    return dict(cand_half=dict(th, flops=2.0 * Cn * d * d,
                               fraction_of_f32_mfma_peak=round(2.0 * Cn * d * d / (th['median_ms'] * 1e-3) / PEAK_F32, 5)),
                scores_shared=dict(tsh, valu_ops=ops, ns_per_pair=round(sec * 1e9 / (B * Cn), 4),
                                   fraction_of_f32_vector_peak=round(ops / sec / PEAK_F32, 5),
                                   fraction_of_unpacked_unfused_issue_rate=round(ops / sec / (PEAK_F32 / 4), 5)))


def measure(model, st, warm, B, cat, reps, k=10):
    dev = model.device
    lo = warm * BS
    src = torch.as_tensor(st['src'][lo:lo + B]).to(dev)
    when = float(st['ts'][lo + BS])
    ts = torch.full((B,), when, dtype=torch.float64, device=dev)
    Cn = cat.numel()
    snap = model.embed_catalogue(cat, when)
    a, b = model.recommend(src, ts, cat, k), model.recommend(src, ts, snap, k)   # warm-up of both forms, and their agreement
    equal = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                for x, y in zip(a, b))
    out = dict(B=B, C=Cn, pairs=B * Cn, lists_equal_bit_for_bit=equal)
    out['recommend_tensors'] = stats([timed(lambda: model.recommend(src, ts, cat, k)) for _ in range(reps)])
    out['embed_catalogue'] = stats([timed(lambda: model.embed_catalogue(cat, when)) for _ in range(reps)])
    out['recommend_snapshot'] = stats([timed(lambda: model.recommend(src, ts, snap, k)) for _ in range(reps)])
    out.update(kernels_alone(model, B, Cn, reps))
    t0, t1, t2 = (out[n]['median_ms'] for n in ('recommend_tensors', 'embed_catalogue', 'recommend_snapshot'))
    out['tensors_over_snapshot'] = round(t0 / t2, 2)
    out['tensors_over_embed_plus_snapshot'] = round(t0 / (t1 + t2), 2)
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
    ap.add_argument('--warm', type=int, default=40, help='streamed batches of 200 events before the measurement')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'recommend_snapshot_v1.json'))
    a = ap.parse_args()
    model, st = setup(a.warm)
    c = bench.C2
    dev = model.device
    items = torch.arange(c['n_u'] + 1, c['n_u'] + c['n_i'] + 1, dtype=torch.int64, device=dev)   # all destinations
    nodes = torch.arange(1, model.n_nodes, dtype=torch.int64, device=dev)                        # all node ids
    out = dict(workload="C2-shaped stream, d 172, K 10, 'bin' hits, k 10, every query at one time", reps=a.reps,
               warm_batches=a.warm, clocks=clocks())
    for name, B, cat in (('B200_destinations', 200, items), ('B1_destinations', 1, items), ('B200_all_nodes', 200, nodes),
                         ('B1_all_nodes', 1, nodes)):
        out[name] = measure(model, st, a.warm, B, cat, a.reps)
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    out['clocks_after'] = clocks().get('engine_clock_now_mhz')
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
