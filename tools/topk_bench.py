#!/usr/bin/env python3
"""Top-k selection measurements (one JSON line per shape, all written to profiles/topk_bench_v1.json): tg_topk_rows with
the library-chosen segment count against the torch formulation of the same contract,

    s = scores.masked_fill(~(mask & (ids != 0) & isfinite(scores)), -inf);  v, c = torch.topk(s, k);  ids.gather(1, c)

(which fixes no order among equal scores and needs the masked temporaries), on per-row int64 ids and a uint8 mask:
  (B 1024, C 1000, k 10)   many short rows, one segment each
  (B 200, C 10000, k 10)   an evaluation batch over a catalogue
  (B 1, C 2^20, k 64)      one long row: segments, then the merge launch
Both are timed in this run on this device with HIP events after warm-up, alternating, `--reps` samples of `--inner` calls
each (median, min, max of the per-call time).  bytes = B C (4 + 8 + 1): the one pass over scores, ids and mask the
kernel's design claims; achieved bytes/s = bytes / median time, quoted against the 8 TB/s HBM peak.  Inputs of these
sizes fit the 256 MiB Infinity Cache, so the rate is a rate out of cache, not out of HBM, wherever bytes < 256 MiB.
The two are also compared: equal score bits in every position (ids may differ among equal scores in torch's).

    python tools/topk_bench.py [--reps R] [--inner N] [--out profiles/topk_bench_v1.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from www2023tiger_amd._lib import check, lib, ptr  # noqa: E402
from www2023tiger_amd.hip_ops import stream_ptr  # noqa: E402

PEAK_HBM = 8.0e12
SHAPES = [(1024, 1000, 10), (200, 10000, 10), (1, 1 << 20, 64)]


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
    return dict(median_us=round(1e3 * statistics.median(v), 3), min_us=round(1e3 * min(v), 3), max_us=round(1e3 * max(v), 3))


def measure(B, C, k, reps, inner):
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(B + C)
    scores = torch.randn(B, C, generator=g).to(dev)
    ids = torch.randint(1, 1 << 40, (B, C), generator=g).to(dev)
    ids[torch.rand(B, C, generator=g).to(dev) < 0.02] = 0
    mask = (torch.rand(B, C, generator=g) > 0.1).to(dev).to(torch.uint8)
    o_ids = torch.empty(B, k, dtype=torch.int64, device=dev)
    o_sc = torch.empty(B, k, dtype=torch.float32, device=dev)
    o_col = torch.empty(B, k, dtype=torch.int32, device=dev)
    nv = torch.empty(B, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    nbytes = int(lib.tg_topk_rows_workspace_bytes(B, C, k, 0))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    s = stream_ptr(dev)

    def ours():
        for _ in range(inner):
            check(lib.tg_topk_rows(B, C, k, ptr(scores), C, ptr(ids), 0, ptr(mask), 0, ptr(o_ids), ptr(o_sc), ptr(o_col), ptr(nv),
                                   ptr(bad), ptr(ws), ws.numel(), s), 'tg_topk_rows')

    def torch_form():
        out = None
        for _ in range(inner):
            keep = mask.bool() & (ids != 0) & torch.isfinite(scores)
            v, c = torch.topk(scores.masked_fill(~keep, float('-inf')), k, dim=1)
            out = (ids.gather(1, c), v, keep.sum(1))
        return out

    ours()
    ref = torch_form()
    same_scores = bool(torch.equal(o_sc.view(torch.int32), ref[1].view(torch.int32)))
    same_ids = float((o_ids == ref[0]).double().mean())
    t_ours, t_torch = [], []
    for _ in range(reps):  # alternating
        t_ours.append(timed(ours))
        t_torch.append(timed(torch_form))
    a, b = stats(t_ours, inner), stats(t_torch, inner)
    moved = B * C * (4 + 8 + 1)
    rate = moved / (a['median_us'] * 1e-6)
    return dict(B=B, C=C, k=k, n_seg=max(1, nbytes // (B * (8 * k + 8))), bytes=moved, tg_topk_rows=a, torch_topk=b,
                achieved_bytes_per_s=round(rate), fraction_of_hbm_peak=round(rate / PEAK_HBM, 4),
                speedup_over_torch=round(b['median_us'] / a['median_us'], 3), score_bits_equal=same_scores,
                ids_equal_share=round(same_ids, 6), fits_infinity_cache=moved < (256 << 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=50, help='calls per timed sample')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'topk_bench_v1.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'topk_bench measures on the GPU'
    p = torch.cuda.get_device_properties(0)
    lines = [json.dumps(dict(device=p.name, compute_units=p.multi_processor_count, reps=a.reps, inner=a.inner,
                             ids='int64 per row', mask='uint8', timer='HIP events around `inner` calls'))]
    for B, C, k in SHAPES:
        lines.append(json.dumps(measure(B, C, k, a.reps, a.inner)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
