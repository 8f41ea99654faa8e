#!/usr/bin/env python3
"""Embedding nearest-neighbour measurements (one JSON line per shape, all written to profiles/knn_v1.json): hip_ops.knn_rows
(tg_knn_rows: selection on the MFMA accumulators, no [Q, C] matrix) against the form a user has without it,

    s = torch.matmul(q[i0:i1], c.T);  hip_ops.topk_rows(s, ids, k)

chunked over Q so that the float32 matrix of a chunk stays at or below `--matrix-bytes` (1 GiB).  The sweep is
Q in {1, 64, 1024} x C in {65536, 1048576} x d in {172, 256} x k in {10, 64}, standard normal operands, ids = column + 1.
Both forms are timed in this run on this device with HIP events after warm-up, alternating, `--reps` samples of `inner`
calls each (inner chosen per shape so that a sample lasts about `--sample-ms`); median, min and max of the per-call time.
Per shape: the fraction of the 157.3 TF float32 matrix peak (2 Q C d FLOP / median), catalogue bytes per second (C d 4 bytes
per call - one logical pass; every query tile re-reads the catalogue through the caches, so this is NOT an HBM rate), the
peak extra device memory of one call of each form (torch.cuda.max_memory_allocated above the operands), and the share of
list positions where the two forms name the same id (the vendor GEMM's bits are not the fmaf chain's, so near-ties may
swap).  No threshold is set: the file records what came out, including the shapes where the fused form loses.

    python tools/knn_bench.py [--reps R] [--sample-ms MS] [--out profiles/knn_v1.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from www2023tiger_amd import hip_ops  # noqa: E402
from www2023tiger_amd._lib import lib  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
QS, CS, DS, KS = (1, 64, 1024), (65536, 1048576), (172, 256), (10, 64)


def timed(fn, inner):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def peak_extra(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def measure(q, c, ids, k, reps, sample_ms, matrix_bytes):
    Q, d = q.shape
    C = c.shape[0]
    rows = max(1, min(Q, matrix_bytes // (4 * C)))

    def fused():
        return hip_ops.knn_rows(q, c, k)

    def matmul_topk():
        outs = []
        for i0 in range(0, Q, rows):
            outs.append(hip_ops.topk_rows(torch.matmul(q[i0:i0 + rows], c.T), ids, k)['ids'])
        return outs

    a = fused()
    b = torch.cat(matmul_topk())
    same = float((a['ids'] == b).double().mean())
    mem_f, mem_m = peak_extra(fused), peak_extra(matmul_topk)
    inner = max(1, min(200, int(sample_ms / max(timed(fused, 1), 1e-3))))
    t_f, t_m = [], []
    for _ in range(reps):  # alternating
        t_f.append(timed(fused, inner))
        t_m.append(timed(matmul_topk, inner))
    sf, sm = stats(t_f), stats(t_m)
    flop = 2.0 * Q * C * d
    n_split = int(lib.tg_knn_rows_workspace_bytes(Q, C, k, 0)) // (Q * (8 * k + 8))
    return dict(Q=Q, C=C, d=d, k=k, n_split=n_split, inner=inner, knn_rows=sf, matmul_topk_rows=sm, matmul_chunk_rows=rows,
                fraction_of_f32_matrix_peak=round(flop / (sf['median_ms'] * 1e-3) / PEAK_F32_MATRIX, 4),
                matmul_fraction_of_f32_matrix_peak=round(flop / (sm['median_ms'] * 1e-3) / PEAK_F32_MATRIX, 4),
                catalogue_bytes_per_s=round(4.0 * C * d / (sf['median_ms'] * 1e-3)),
                speedup_over_matmul_topk=round(sm['median_ms'] / sf['median_ms'], 3),
                peak_extra_bytes=dict(knn_rows=mem_f, matmul_topk_rows=mem_m), ids_equal_share=round(same, 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sample-ms', type=float, default=40.0, help='target length of one timed sample')
    ap.add_argument('--matrix-bytes', type=int, default=1 << 30, help="largest [rows, C] float32 chunk of the matmul form")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'knn_v1.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'knn_bench measures on the GPU'
    dev = torch.device('cuda', 0)
    p = torch.cuda.get_device_properties(0)
    lines = [json.dumps(dict(device=p.name, compute_units=p.multi_processor_count, reps=a.reps, sample_ms=a.sample_ms,
                             matrix_bytes=a.matrix_bytes, operands='standard normal float32, ids = column + 1',
                             timer='HIP events around `inner` calls, the two forms alternating'))]
    g = torch.Generator(device=dev).manual_seed(1)
    for d in DS:
        for C in CS:
            c = torch.randn(C, d, generator=g, device=dev)
            ids = torch.arange(1, C + 1, dtype=torch.int64, device=dev)
            for Q in QS:
                q = torch.randn(Q, d, generator=g, device=dev)
                for k in KS:
                    lines.append(json.dumps(measure(q, c, ids, k, a.reps, a.sample_ms, a.matrix_bytes)))
                    print(lines[-1], flush=True)
            del c, ids
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
